// C ABI of the MI355X-native budgeted-KV attention path (see include/easykv_hip.h): the entry points, and the launch loop that runs what
// the planner (ekv_plan.cpp) resolved.  The bank utility kernels are in ekv_bank_ops.hip.
#include "ekv_common.h"
#include "ekv_kernels.h"
#include "ekv_plan.h"

// A launch failure must be reported as THIS call's, not as whatever sticky-free error an earlier, unrelated runtime call of the
// thread left behind: every entry point drops the stale last-error state first, then reports its own launches.
static inline void drop_stale_error() { (void)hipGetLastError(); }
static inline int launch_code(hipError_t e) { return e == hipSuccess ? EKV_OK : EKV_E_LAUNCH; }

// Body of ekv_step_attend and its kin: the resolved call, the pointers, then the plan's launch sequence.
static int call_attend(const EkvCall& c, const void* q, const void* k_new, const void* v_new, void* out, int32_t* evict_ids,
                       const float* rope_cos, const float* rope_sin, void* workspace, size_t workspace_bytes, void* stream) {
  EkvResolved r;
  if (int e = resolve_call(c, &r)) return e;
  const ekv_bank* bank = r.bank;
  const ekv_step* st = r.step;
  const EkvSeqTable* tb = r.tb;
  const EkvStepPlan& P = r.plan;
  if (!q || !k_new || !v_new || !out || !workspace || (st->rope_on_read && (!rope_cos || !rope_sin))) return EKV_E_ARG;
  if (P.bytes > workspace_bytes) return EKV_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = st->q_len, D = bank->head_dim, lc = st->layer_count;
  char* const ws = static_cast<char*>(workspace);
  auto f32 = [&](int64_t off) { return off < 0 ? nullptr : reinterpret_cast<float*>(ws + off); };
  auto f16 = [&](int64_t off) { return off < 0 ? nullptr : reinterpret_cast<__half*>(ws + off); };

  EkvAttnArgs aa{};
  aa.k = static_cast<const __half*>(bank->k);
  aa.v = static_cast<const __half*>(bank->v);
  aa.k_w = static_cast<__half*>(bank->k);
  aa.v_w = static_cast<__half*>(bank->v);
  aa.slot_of_pos = bank->slot_of_pos;
  aa.q = static_cast<const __half*>(q);
  aa.k_new = static_cast<const __half*>(k_new);
  aa.v_new = static_cast<const __half*>(v_new);
  aa.logits = f32(P.logits);
  aa.partials = f32(P.partials);
  aa.rope_cos = st->rope_on_read ? rope_cos : nullptr;
  aa.rope_sin = st->rope_on_read ? rope_sin : nullptr;
  aa.q_rot_hi = f16(P.q_rot);
  aa.q_rot_lo = aa.q_rot_hi ? aa.q_rot_hi + (size_t)lc * bank->n_q_heads * n * D : nullptr;
  aa.out_direct = (P.fold_in_kernel || P.fold_in_decode) ? static_cast<__half*>(out) : nullptr;
  aa.arrive = P.fold_in_decode ? bank->arrive + (size_t)st->layer_begin * bank->n_kv_heads : nullptr;
  aa.row_stats = f32(P.row_stats);
  aa.stats = f32(P.stats);
  aa.colsum = f32(P.colsum);
  aa.n_col_parts = P.n_col_parts;
  aa.n_q_heads = bank->n_q_heads;
  aa.n_kv_heads = bank->n_kv_heads;
  aa.cap = bank->cap;
  aa.n_slots = st->n_slots;
  aa.q_len = n;
  aa.n_split = P.n_split;
  aa.rows_per_split = P.rows_per_split;
  aa.t_pad = P.t_pad;
  aa.layer_begin = st->layer_begin;
  aa.causal = st->causal;
  aa.qb_rows = P.qb_rows;
  aa.n_qblocks = P.n_qblocks;
  aa.sm_div = st->sm_div;
  aa.softcap = c.capped ? c.softcap : 0.f;
  aa.q_keep = f16(P.q_keep);
  aa.phys_extent = P.phys_extent;
  aa.l_pad = P.l_pad;
  aa.q_ts = P.strides[0], aa.q_hs = P.strides[1], aa.kv_ts = P.strides[2], aa.kv_hs = P.strides[3], aa.o_ts = P.strides[4], aa.o_hs = P.strides[5];

  EkvScoreArgs sa = score_args(bank, st, P);
  sa.slot_of_pos = bank->slot_of_pos;
  sa.score_sum = bank->score_sum;
  sa.score_sq = bank->score_sq;
  sa.score_cnt = bank->score_cnt;
  sa.logits = aa.logits;
  sa.partials = aa.partials;
  sa.tova_row = f32(P.tova_row);
  sa.colsum = aa.colsum;
  sa.row_stats = aa.row_stats;
  // quantised rows: the row scales / block exponents (they share the storage of stats / colsum, which a decode step — all a quantised
  // plan can be — never has)
  if (c.rows == EKV_ROWS_kv8) aa.k_scale = static_cast<float*>(c.planes.k_aux), aa.v_scale = static_cast<float*>(c.planes.v_aux);
  if (c.rows == EKV_ROWS_kv4 || c.rows == EKV_ROWS_kv6) aa.k_exp = static_cast<uint8_t*>(c.planes.k_aux), aa.v_exp = static_cast<uint8_t*>(c.planes.v_aux);
  if (c.rows == EKV_ROWS_kv84) aa.k_scale = static_cast<float*>(c.planes.k_aux), aa.v_exp = static_cast<uint8_t*>(c.planes.v_aux);
  if (c.rows == EKV_ROWS_kv164) aa.v_exp = static_cast<uint8_t*>(c.planes.v_aux);      // (the keys: bank->k, as resolve_call left it)
  sa.out = static_cast<__half*>(out);
  sa.evict_ids = evict_ids;
  sa.big_rows = f32(P.big_rows);
  sa.slot_state = bank->slot_state;      // (word [3] of a head: threshold hint of the logits-in-LDS chunk kernel, whatever the layout)
  if (P.slot_rows) {
    sa.birth = bank->birth;
    sa.cnt_tail = ekv_cnt_tail(bank);
    sa.slot_tail_ok = P.slot_tail_ok;
  }

  const bool bf16 = P.bf16 != 0;
  const EkvRows rows = static_cast<EkvRows>(P.rows);
  const bool capped = P.capped != 0;
  const float* const sinks = P.sink ? c.sinks : nullptr;      // (a sink plan: every attention launch and the split path's scorer run the sink instances)
  // (a window plan: the attention launches run the window instances — with sinks the sink + window ones — and stamp the appended rows'
  // token positions; the scorers behind them read logits, partials, row statistics and column sums and are the plain / sink ones)
  const bool window = P.window != 0;
  const EkvWinArgs win = window ? EkvWinArgs{c.win->tok_pos, c.win->windows, c.win->q_pos0} : EkvWinArgs{};
  // (a heads plan: the split kernel and the split path's scorer run the heads instances, which read each head's row count from the table)
  const bool heads = P.heads != 0;
  const EkvHeadsArgs hd = heads ? EkvHeadsArgs{c.hd->rows, c.hd->grow} : EkvHeadsArgs{};
  drop_stale_error();
  for (int i = 0; i < P.n_list; ++i) {
    const EkvLaunch& L = P.list[i];
    sa.skip_fold = L.skip_fold;
    hipError_t e = hipSuccess;
    // (a window plan: the decode launches and the 16x16x32 chunk kernel, the only kernels with window instances)
    if (window && (L.kind == EKV_RUN_CHUNK_LDS || L.kind == EKV_RUN_RESIDENT || L.kind == EKV_RUN_FLUSH || (L.kind == EKV_RUN_CHUNK && P.wide))) return EKV_E_UNSUPPORTED;
    // (a quantised plan is a decode plan: the decode attention launches and the scorers behind them, which read no K/V element)
    if (rows != EKV_ROWS_kv16 && (L.kind == EKV_RUN_CHUNK_LDS || L.kind == EKV_RUN_RESIDENT || L.kind == EKV_RUN_CHUNK || L.kind == EKV_RUN_FLUSH)) return EKV_E_UNSUPPORTED;
    // (a capped plan: the decode launches and the 16x16x32 chunk kernel, the only kernels with capped instances)
    // (a sink plan likewise)
    if (sinks && (L.kind == EKV_RUN_CHUNK_LDS || L.kind == EKV_RUN_RESIDENT || L.kind == EKV_RUN_FLUSH || (L.kind == EKV_RUN_CHUNK && P.wide))) return EKV_E_UNSUPPORTED;
    if (heads && L.kind != EKV_RUN_DECODE && L.kind != EKV_RUN_FOLD && L.kind != EKV_RUN_DECODE_SCORE) return EKV_E_UNSUPPORTED;
    if (capped && (L.kind == EKV_RUN_CHUNK_LDS || L.kind == EKV_RUN_RESIDENT || L.kind == EKV_RUN_FLUSH || (L.kind == EKV_RUN_CHUNK && P.wide))) return EKV_E_UNSUPPORTED;
    switch (L.kind) {
      case EKV_RUN_FUSED_DECODE:
        aa.fused_order = P.fused_order;      // (shares its storage with score_tail, which only chunk launches set)
        e = window ? ekv_launch_decode_fused_win(aa, sa, sinks, win, D, lc, P.fused_nw, s, bf16)
          : sinks ? ekv_launch_decode_fused_sink(aa, sa, sinks, D, lc, P.fused_nw, s, bf16)
                  : ekv_launch_decode_fused(aa, sa, tb, D, lc, P.fused_nw, s, bf16, rows, capped);
        break;
      case EKV_RUN_CHUNK_LDS: e = ekv_launch_chunk_lds(aa, sa, D, lc, s, bf16); break;
      case EKV_RUN_RESIDENT: e = ekv_launch_attn_resident(aa, sa, lc, s, bf16); break;
      case EKV_RUN_DECODE:
        e = heads ? ekv_launch_attn_decode_heads(aa, hd, D, lc, s, bf16)
          : window ? ekv_launch_attn_decode_win(aa, sinks, win, D, lc, s, bf16)
          : sinks ? ekv_launch_attn_decode_sink(aa, sinks, D, lc, s, bf16) : ekv_launch_attn_decode(aa, tb, D, lc, s, bf16, rows, capped);
        break;
      case EKV_RUN_CHUNK:
        e = window ? ekv_launch_attn_chunk_win(aa, sinks, win, D, lc, P.two_pass, s, L.fuse ? &sa : nullptr, bf16)
          : sinks ? ekv_launch_attn_chunk_sink(aa, sinks, D, lc, P.two_pass, s, L.fuse ? &sa : nullptr, bf16)
                  : ekv_launch_attn_chunk(aa, D, lc, P.wide, P.two_pass, s, L.fuse ? &sa : nullptr, L.passes, L.tail ? &sa : nullptr, bf16, capped);
        break;
      case EKV_RUN_FLUSH: {
        EkvAttnArgs a2 = aa;
        a2.q = aa.q_keep;
        a2.q_keep = nullptr;
        a2.new_in_cache = 1;
        a2.q_ts = D, a2.q_hs = n * D;      // (the kept copies are dense)
        if (P.flush_unsplit) {
          a2.n_stat_parts = P.n_split;
          a2.n_split = 1;
          a2.rows_per_split = P.t_pad;
        }
        e = ekv_launch_attn_chunk(a2, D, lc, P.wide, true, s, nullptr, L.passes, L.tail ? &sa : nullptr, bf16);
        break;
      }
      case EKV_RUN_FOLD: e = ekv_launch_fold(sa, lc, s, bf16); break;
      case EKV_RUN_RANGE:
        e = ekv_launch_range_evict(bank, st, tb, evict_ids, s);
        break;
      case EKV_RUN_DECODE_SCORE:
        e = heads ? ekv_launch_decode_score_heads(sa, hd, lc, s, bf16)
          : sinks ? ekv_launch_decode_score_sink(sa, sinks, lc, s, bf16) : ekv_launch_decode_score(sa, tb, lc, s, bf16);
        break;
      case EKV_RUN_TOVA_MEAN: e = sinks ? ekv_launch_tova_headmean_sink(sa, sinks, lc, s) : ekv_launch_tova_headmean(sa, lc, s); break;
      // (a pooled plan: the EKV_POOL instances of the generic scorer, the struct's two words as the kernel's last argument)
      // (an adaptive plan: rank, allot, select — the EKV_ADA instances twice around the allot kernel.  The select phase reads the score rows
      // the rank phase wrote back and must do none of the scorer's attention-side work again: skip_fold = 1 with accumulate = 0 makes
      // step 0 of ekv_score_select_body fold nothing (`nothing_to_fold`: no partials read, no output written), and accumulate = 0 keeps
      // step 2 off the logits / column sums (neither the wide sweep nor the column-sum path runs: the rows are loaded as the bank holds
      // them, and nothing is added a second time).  A change to those two conditions must keep both true for this launch.)
      case EKV_RUN_SCORE_SELECT:
        if (P.adaptive) {
          EkvAdaArgs ad{c.ada->radius, c.ada->op, c.ada->evict_min, c.ada->evict_max, 0, P.t_pad, reinterpret_cast<uint32_t*>(ws + P.ada_keys),
                        reinterpret_cast<uint8_t*>(ws + P.ada_cls), c.ada->n_evict_out};
          e = ekv_launch_score_select_ada(sa, ad, lc, s, bf16);
          if (e == hipSuccess) e = ekv_launch_score_allot(sa, ad, lc, s);
          EkvScoreArgs sel = sa;
          sel.accumulate = 0, sel.skip_fold = 1;
          ad.phase = 1;
          if (e == hipSuccess) e = ekv_launch_score_select_ada(sel, ad, lc, s, bf16);
          break;
        }
        e = P.pooled ? ekv_launch_score_select_pool(sa, EkvPoolArgs{c.pool->radius, c.pool->op}, lc, s, bf16) : ekv_launch_score_select(sa, lc, s, bf16);
        break;
      // long calls (L.passes: the plain plan keeps its rows in scratch)
      case EKV_RUN_LONG_FOLD: e = ekv_launch_long_fold(sa, L.passes != 0, lc, s, bf16); break;
      case EKV_RUN_LONG_SCORE:
        e = ekv_launch_score_long(sa, P.key_rows < 0 ? nullptr : reinterpret_cast<uint32_t*>(ws + P.key_rows), L.passes != 0, lc, s);
        break;
    }
    if (e != hipSuccess) return EKV_E_LAUNCH;
  }
  return EKV_OK;
}

extern "C" {

// ---- the entry points of the step family: one or two lines over the four internals above
size_t ekv_workspace_bytes_typed(const ekv_bank* bank, const ekv_step* step, int32_t dtype) { return call_workspace_bytes(step_call(bank, step, dtype)); }
size_t ekv_workspace_bytes(const ekv_bank* bank, const ekv_step* step) { return call_workspace_bytes(step_call(bank, step, EKV_DTYPE_F16)); }

int ekv_step_plan(const ekv_bank* bank, const ekv_step* st, int32_t* n_split, int32_t* fused) { return call_plan(bank, st, n_split, fused); }

int ekv_step_info_typed(const ekv_bank* bank, const ekv_step* st, int32_t dtype, int32_t* info, int32_t n_info) {
  return call_info(step_call(bank, st, dtype), info, n_info);
}
int ekv_step_info(const ekv_bank* bank, const ekv_step* st, int32_t* info, int32_t n_info) {
  return call_info(step_call(bank, st, EKV_DTYPE_F16), info, n_info);
}

// resident rows of the one-launch decode step (include/easykv_hip.h, "resident rows")
int ekv_set_resident_bytes(int64_t bytes) {
  ekv_resident_set_budget_bytes(bytes);
  return EKV_OK;
}
int ekv_step_resident_rows(const ekv_bank* bank, const ekv_step* st, int32_t dtype) { return call_resident_rows(step_call(bank, st, dtype)); }

int ekv_step_check_typed(const ekv_bank* bank, const ekv_step* st, int32_t dtype) { return call_check(step_call(bank, st, dtype)); }
int ekv_step_check(const ekv_bank* bank, const ekv_step* st) { return call_check(step_call(bank, st, EKV_DTYPE_F16)); }

int ekv_step_attend(const ekv_bank* bank, const ekv_step* st, const void* q, const void* k_new, const void* v_new,
                    void* out, int32_t* evict_ids, const float* rope_cos, const float* rope_sin, void* workspace,
                    size_t workspace_bytes, void* stream) {
  return call_attend(step_call(bank, st, EKV_DTYPE_F16), q, k_new, v_new, out, evict_ids, rope_cos, rope_sin, workspace, workspace_bytes, stream);
}
int ekv_step_attend_typed(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const void* q, const void* k_new,
                          const void* v_new, void* out, int32_t* evict_ids, const float* rope_cos, const float* rope_sin,
                          void* workspace, size_t workspace_bytes, void* stream) {
  return call_attend(step_call(bank, st, dtype), q, k_new, v_new, out, evict_ids, rope_cos, rope_sin, workspace, workspace_bytes, stream);
}

// long score rows (include/easykv_hip.h, "long score rows"): the _typed calls with the long-row scorer where the plan would end in the generic one
int ekv_long_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype) { return call_check(long_call(bank, st, dtype)); }
int ekv_long_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, int32_t* info, int32_t n_info) {
  return call_info(long_call(bank, st, dtype), info, n_info);
}
size_t ekv_long_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype) { return call_workspace_bytes(long_call(bank, st, dtype)); }
int ekv_long_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const void* q, const void* k_new, const void* v_new,
                         void* out, int32_t* evict_ids, const float* rope_cos, const float* rope_sin, void* workspace,
                         size_t workspace_bytes, void* stream) {
  return call_attend(long_call(bank, st, dtype), q, k_new, v_new, out, evict_ids, rope_cos, rope_sin, workspace, workspace_bytes, stream);
}

// soft-capped attention logits (include/easykv_hip.h, "soft-capped logits"): the _typed calls with a cap
int ekv_cap_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, float softcap) { return call_check(cap_call(bank, st, dtype, softcap)); }
int ekv_cap_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, float softcap, int32_t* info, int32_t n_info) {
  return call_info(cap_call(bank, st, dtype, softcap), info, n_info);
}
size_t ekv_cap_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, float softcap) {
  return call_workspace_bytes(cap_call(bank, st, dtype, softcap));
}
int ekv_cap_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, float softcap, const void* q, const void* k_new, const void* v_new,
                        void* out, int32_t* evict_ids, const float* rope_cos, const float* rope_sin, void* workspace,
                        size_t workspace_bytes, void* stream) {
  return call_attend(cap_call(bank, st, dtype, softcap), q, k_new, v_new, out, evict_ids, rope_cos, rope_sin, workspace, workspace_bytes, stream);
}
int ekv_softcap_eval(const float* x, int64_t n, float sm_div, float cap, float* out, void* stream) {
  if (n < 0 || (n > 0 && (!x || !out)) || !(cap > 0.f && cap <= 3.0e38f) || !(sm_div > 0.f)) return EKV_E_ARG;
  drop_stale_error();
  return launch_code(ekv_launch_softcap_eval(x, n, sm_div, cap, out, static_cast<hipStream_t>(stream)));
}

// attention sinks (include/easykv_hip.h, "attention sinks"): the _typed calls with the sinks behind the element type
int ekv_sink_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const float* sinks) { return call_check(sink_call(bank, st, dtype, sinks)); }
int ekv_sink_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const float* sinks, int32_t* info, int32_t n_info) {
  return call_info(sink_call(bank, st, dtype, sinks), info, n_info);
}
size_t ekv_sink_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const float* sinks) {
  return call_workspace_bytes(sink_call(bank, st, dtype, sinks));
}
int ekv_sink_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const float* sinks, const void* q, const void* k_new,
                         const void* v_new, void* out, int32_t* evict_ids, const float* rope_cos, const float* rope_sin, void* workspace,
                         size_t workspace_bytes, void* stream) {
  return call_attend(sink_call(bank, st, dtype, sinks), q, k_new, v_new, out, evict_ids, rope_cos, rope_sin, workspace, workspace_bytes, stream);
}

// sliding windows (include/easykv_hip.h, "sliding windows"): the _typed calls with the window struct behind the element type
int ekv_win_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_win* win) { return call_check(win_call(bank, st, dtype, win)); }
int ekv_win_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_win* win, int32_t* info, int32_t n_info) {
  return call_info(win_call(bank, st, dtype, win), info, n_info);
}
size_t ekv_win_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_win* win) {
  return call_workspace_bytes(win_call(bank, st, dtype, win));
}
int ekv_win_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_win* win, const void* q, const void* k_new,
                        const void* v_new, void* out, int32_t* evict_ids, const float* rope_cos, const float* rope_sin, void* workspace,
                        size_t workspace_bytes, void* stream) {
  return call_attend(win_call(bank, st, dtype, win), q, k_new, v_new, out, evict_ids, rope_cos, rope_sin, workspace, workspace_bytes, stream);
}

// pooled selection (include/easykv_hip.h, "pooled selection"): the _typed calls with the pooling struct behind the element type
int ekv_pool_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_pool* pool) { return call_check(pool_call(bank, st, dtype, pool)); }
int ekv_pool_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_pool* pool, int32_t* info, int32_t n_info) {
  return call_info(pool_call(bank, st, dtype, pool), info, n_info);
}
size_t ekv_pool_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_pool* pool) {
  return call_workspace_bytes(pool_call(bank, st, dtype, pool));
}
int ekv_pool_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_pool* pool, const void* q, const void* k_new,
                         const void* v_new, void* out, int32_t* evict_ids, const float* rope_cos, const float* rope_sin, void* workspace,
                         size_t workspace_bytes, void* stream) {
  return call_attend(pool_call(bank, st, dtype, pool), q, k_new, v_new, out, evict_ids, rope_cos, rope_sin, workspace, workspace_bytes, stream);
}

// adaptive head budgets (include/easykv_hip.h, "adaptive head budgets"): the _typed calls with the budget struct behind the element type
int ekv_ada_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_ada* ada) { return call_check(ada_call(bank, st, dtype, ada)); }
int ekv_ada_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_ada* ada, int32_t* info, int32_t n_info) {
  return call_info(ada_call(bank, st, dtype, ada), info, n_info);
}
size_t ekv_ada_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_ada* ada) {
  return call_workspace_bytes(ada_call(bank, st, dtype, ada));
}
int ekv_ada_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_ada* ada, const void* q, const void* k_new,
                        const void* v_new, void* out, int32_t* evict_ids, const float* rope_cos, const float* rope_sin, void* workspace,
                        size_t workspace_bytes, void* stream) {
  return call_attend(ada_call(bank, st, dtype, ada), q, k_new, v_new, out, evict_ids, rope_cos, rope_sin, workspace, workspace_bytes, stream);
}

// FP8 K/V storage (include/easykv_hip.h, "kv8")
int ekv_kv8_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv8* q8) { return call_check(kv8_call(bank, st, dtype, q8)); }
int ekv_kv8_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv8* q8, int32_t* info, int32_t n_info) {
  return call_info(kv8_call(bank, st, dtype, q8), info, n_info);
}
size_t ekv_kv8_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv8* q8) {
  return call_workspace_bytes(kv8_call(bank, st, dtype, q8));
}
int ekv_kv8_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv8* q8, const void* q, const void* k_new,
                        const void* v_new, void* out, int32_t* evict_ids, const float* rope_cos, const float* rope_sin,
                        void* workspace, size_t workspace_bytes, void* stream) {
  return call_attend(kv8_call(bank, st, dtype, q8), q, k_new, v_new, out, evict_ids, rope_cos, rope_sin, workspace, workspace_bytes, stream);
}

// decode steps over KV heads of different lengths (include/easykv_hip.h, ekv_heads)
int ekv_heads_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_heads* heads) { return call_check(heads_call(bank, st, dtype, heads)); }
int ekv_heads_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_heads* heads, int32_t* info, int32_t n_info) {
  return call_info(heads_call(bank, st, dtype, heads), info, n_info);
}
size_t ekv_heads_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_heads* heads) {
  return call_workspace_bytes(heads_call(bank, st, dtype, heads));
}
int ekv_heads_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_heads* heads, const void* q, const void* k_new,
                          const void* v_new, void* out, int32_t* evict_ids, void* workspace, size_t workspace_bytes, void* stream) {
  return call_attend(heads_call(bank, st, dtype, heads), q, k_new, v_new, out, evict_ids, nullptr, nullptr, workspace, workspace_bytes, stream);
}

// batched decode steps (include/easykv_hip.h, ekv_seq)
int ekv_batch_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_seq* seqs, int32_t n_seq) {
  return call_check(batch_call(bank, st, dtype, seqs, n_seq));
}
int ekv_batch_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_seq* seqs, int32_t n_seq, int32_t* info,
                        int32_t n_info) {
  return call_info(batch_call(bank, st, dtype, seqs, n_seq), info, n_info);
}
size_t ekv_batch_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_seq* seqs, int32_t n_seq) {
  return call_workspace_bytes(batch_call(bank, st, dtype, seqs, n_seq));
}
int ekv_batch_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_seq* seqs, int32_t n_seq, const void* q,
                          const void* k_new, const void* v_new, void* out, int32_t* evict_ids, void* workspace, size_t workspace_bytes,
                          void* stream) {
  return call_attend(batch_call(bank, st, dtype, seqs, n_seq), q, k_new, v_new, out, evict_ids, nullptr, nullptr, workspace, workspace_bytes, stream);
}

// batched decode steps on a kv8 bank (include/easykv_hip.h, "kv8 batches")
int ekv_kv8_batch_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv8* q8, const ekv_seq* seqs, int32_t n_seq) {
  return call_check(kv8_batch_call(bank, st, dtype, q8, seqs, n_seq));
}
int ekv_kv8_batch_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv8* q8, const ekv_seq* seqs, int32_t n_seq,
                            int32_t* info, int32_t n_info) {
  return call_info(kv8_batch_call(bank, st, dtype, q8, seqs, n_seq), info, n_info);
}
size_t ekv_kv8_batch_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv8* q8, const ekv_seq* seqs, int32_t n_seq) {
  return call_workspace_bytes(kv8_batch_call(bank, st, dtype, q8, seqs, n_seq));
}
int ekv_kv8_batch_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv8* q8, const ekv_seq* seqs, int32_t n_seq,
                              const void* q, const void* k_new, const void* v_new, void* out, int32_t* evict_ids, void* workspace,
                              size_t workspace_bytes, void* stream) {
  return call_attend(kv8_batch_call(bank, st, dtype, q8, seqs, n_seq), q, k_new, v_new, out, evict_ids, nullptr, nullptr, workspace, workspace_bytes, stream);
}

// MXFP4 K/V storage (include/easykv_hip.h, "kv4")
int ekv_kv4_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv4* q4) { return call_check(kv4_call(bank, st, dtype, q4)); }
int ekv_kv4_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv4* q4, int32_t* info, int32_t n_info) {
  return call_info(kv4_call(bank, st, dtype, q4), info, n_info);
}
size_t ekv_kv4_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv4* q4) {
  return call_workspace_bytes(kv4_call(bank, st, dtype, q4));
}
int ekv_kv4_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv4* q4, const void* q, const void* k_new,
                        const void* v_new, void* out, int32_t* evict_ids, const float* rope_cos, const float* rope_sin,
                        void* workspace, size_t workspace_bytes, void* stream) {
  return call_attend(kv4_call(bank, st, dtype, q4), q, k_new, v_new, out, evict_ids, rope_cos, rope_sin, workspace, workspace_bytes, stream);
}

// batched decode steps on a kv4 bank (include/easykv_hip.h, "kv4 batches")
int ekv_kv4_batch_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv4* q4, const ekv_seq* seqs, int32_t n_seq) {
  return call_check(kv4_batch_call(bank, st, dtype, q4, seqs, n_seq));
}
int ekv_kv4_batch_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv4* q4, const ekv_seq* seqs, int32_t n_seq,
                            int32_t* info, int32_t n_info) {
  return call_info(kv4_batch_call(bank, st, dtype, q4, seqs, n_seq), info, n_info);
}
size_t ekv_kv4_batch_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv4* q4, const ekv_seq* seqs, int32_t n_seq) {
  return call_workspace_bytes(kv4_batch_call(bank, st, dtype, q4, seqs, n_seq));
}
int ekv_kv4_batch_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv4* q4, const ekv_seq* seqs, int32_t n_seq,
                              const void* q, const void* k_new, const void* v_new, void* out, int32_t* evict_ids, void* workspace,
                              size_t workspace_bytes, void* stream) {
  return call_attend(kv4_batch_call(bank, st, dtype, q4, seqs, n_seq), q, k_new, v_new, out, evict_ids, nullptr, nullptr, workspace, workspace_bytes, stream);
}

// MXFP6 K/V storage (include/easykv_hip.h, "kv6"), uniform and batched steps
int ekv_kv6_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv6* q6) { return call_check(kv6_call(bank, st, dtype, q6)); }
int ekv_kv6_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv6* q6, int32_t* info, int32_t n_info) {
  return call_info(kv6_call(bank, st, dtype, q6), info, n_info);
}
size_t ekv_kv6_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv6* q6) {
  return call_workspace_bytes(kv6_call(bank, st, dtype, q6));
}
int ekv_kv6_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv6* q6, const void* q, const void* k_new,
                        const void* v_new, void* out, int32_t* evict_ids, const float* rope_cos, const float* rope_sin,
                        void* workspace, size_t workspace_bytes, void* stream) {
  return call_attend(kv6_call(bank, st, dtype, q6), q, k_new, v_new, out, evict_ids, rope_cos, rope_sin, workspace, workspace_bytes, stream);
}
int ekv_kv6_batch_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv6* q6, const ekv_seq* seqs, int32_t n_seq) {
  return call_check(kv6_batch_call(bank, st, dtype, q6, seqs, n_seq));
}
int ekv_kv6_batch_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv6* q6, const ekv_seq* seqs, int32_t n_seq,
                            int32_t* info, int32_t n_info) {
  return call_info(kv6_batch_call(bank, st, dtype, q6, seqs, n_seq), info, n_info);
}
size_t ekv_kv6_batch_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv6* q6, const ekv_seq* seqs, int32_t n_seq) {
  return call_workspace_bytes(kv6_batch_call(bank, st, dtype, q6, seqs, n_seq));
}
int ekv_kv6_batch_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv6* q6, const ekv_seq* seqs, int32_t n_seq,
                              const void* q, const void* k_new, const void* v_new, void* out, int32_t* evict_ids, void* workspace,
                              size_t workspace_bytes, void* stream) {
  return call_attend(kv6_batch_call(bank, st, dtype, q6, seqs, n_seq), q, k_new, v_new, out, evict_ids, nullptr, nullptr, workspace, workspace_bytes, stream);
}

// FP8-key / MXFP4-value K/V storage (include/easykv_hip.h, "kv84"), uniform and batched steps
int ekv_kv84_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv84* q84) { return call_check(kv84_call(bank, st, dtype, q84)); }
int ekv_kv84_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv84* q84, int32_t* info, int32_t n_info) {
  return call_info(kv84_call(bank, st, dtype, q84), info, n_info);
}
size_t ekv_kv84_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv84* q84) {
  return call_workspace_bytes(kv84_call(bank, st, dtype, q84));
}
int ekv_kv84_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv84* q84, const void* q, const void* k_new,
                         const void* v_new, void* out, int32_t* evict_ids, const float* rope_cos, const float* rope_sin,
                         void* workspace, size_t workspace_bytes, void* stream) {
  return call_attend(kv84_call(bank, st, dtype, q84), q, k_new, v_new, out, evict_ids, rope_cos, rope_sin, workspace, workspace_bytes, stream);
}
int ekv_kv84_batch_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv84* q84, const ekv_seq* seqs, int32_t n_seq) {
  return call_check(kv84_batch_call(bank, st, dtype, q84, seqs, n_seq));
}
int ekv_kv84_batch_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv84* q84, const ekv_seq* seqs, int32_t n_seq,
                             int32_t* info, int32_t n_info) {
  return call_info(kv84_batch_call(bank, st, dtype, q84, seqs, n_seq), info, n_info);
}
size_t ekv_kv84_batch_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv84* q84, const ekv_seq* seqs, int32_t n_seq) {
  return call_workspace_bytes(kv84_batch_call(bank, st, dtype, q84, seqs, n_seq));
}
int ekv_kv84_batch_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv84* q84, const ekv_seq* seqs, int32_t n_seq,
                               const void* q, const void* k_new, const void* v_new, void* out, int32_t* evict_ids, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return call_attend(kv84_batch_call(bank, st, dtype, q84, seqs, n_seq), q, k_new, v_new, out, evict_ids, nullptr, nullptr, workspace, workspace_bytes, stream);
}

// 16-bit-key / MXFP4-value K/V storage (include/easykv_hip.h, "kv164"), uniform and batched steps
int ekv_kv164_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv164* q164) { return call_check(kv164_call(bank, st, dtype, q164)); }
int ekv_kv164_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv164* q164, int32_t* info, int32_t n_info) {
  return call_info(kv164_call(bank, st, dtype, q164), info, n_info);
}
size_t ekv_kv164_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv164* q164) {
  return call_workspace_bytes(kv164_call(bank, st, dtype, q164));
}
int ekv_kv164_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv164* q164, const void* q, const void* k_new,
                          const void* v_new, void* out, int32_t* evict_ids, const float* rope_cos, const float* rope_sin,
                          void* workspace, size_t workspace_bytes, void* stream) {
  return call_attend(kv164_call(bank, st, dtype, q164), q, k_new, v_new, out, evict_ids, rope_cos, rope_sin, workspace, workspace_bytes, stream);
}
int ekv_kv164_batch_step_check(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv164* q164, const ekv_seq* seqs, int32_t n_seq) {
  return call_check(kv164_batch_call(bank, st, dtype, q164, seqs, n_seq));
}
int ekv_kv164_batch_step_info(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv164* q164, const ekv_seq* seqs, int32_t n_seq,
                              int32_t* info, int32_t n_info) {
  return call_info(kv164_batch_call(bank, st, dtype, q164, seqs, n_seq), info, n_info);
}
size_t ekv_kv164_batch_workspace_bytes(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv164* q164, const ekv_seq* seqs, int32_t n_seq) {
  return call_workspace_bytes(kv164_batch_call(bank, st, dtype, q164, seqs, n_seq));
}
int ekv_kv164_batch_step_attend(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv164* q164, const ekv_seq* seqs, int32_t n_seq,
                                const void* q, const void* k_new, const void* v_new, void* out, int32_t* evict_ids, void* workspace,
                                size_t workspace_bytes, void* stream) {
  return call_attend(kv164_batch_call(bank, st, dtype, q164, seqs, n_seq), q, k_new, v_new, out, evict_ids, nullptr, nullptr, workspace, workspace_bytes, stream);
}

// ---- bank conversions (ekv_kv8.hip, ekv_kv4.hip): one argument check for every row format
static int convert_check(const ekv_bank* bank, EkvRows rows, const EkvPlanes& planes, int32_t layer_begin, int32_t layer_count, int32_t extent) {
  if (!bank || !ekv_planes_complete(rows, planes)) return EKV_E_ARG;
  if (bank->n_layers <= 0 || bank->n_kv_heads <= 0 || bank->cap <= 0) return EKV_E_ARG;
  if (int e = check_layers(bank, layer_begin, layer_count)) return e;
  if (extent < 0 || extent > bank->cap) return EKV_E_ARG;
  return ekv_rows_head_dim(rows, bank->head_dim) ? EKV_OK : EKV_E_UNSUPPORTED;
}
static int quantize_check(const ekv_bank* bank, EkvRows rows, const EkvPlanes& planes, int32_t dtype, int32_t layer_begin, int32_t layer_count,
                          int32_t extent) {
  if (dtype != EKV_DTYPE_F16 && dtype != EKV_DTYPE_BF16) return EKV_E_ARG;
  if (int e = convert_check(bank, rows, planes, layer_begin, layer_count, extent)) return e;
  return (bank->k || rows == EKV_ROWS_kv164) && bank->v ? EKV_OK : EKV_E_ARG;      // (kv164 converts V alone)
}
static int dequantize_check(const ekv_bank* bank, EkvRows rows, const EkvPlanes& planes, int32_t out_dtype, int32_t layer_begin,
                            int32_t layer_count, int32_t extent, const void* k_out, const void* v_out) {
  if (out_dtype != EKV_DTYPE_F16 && out_dtype != EKV_DTYPE_BF16 && out_dtype != EKV_DTYPE_F32) return EKV_E_ARG;
  if (int e = convert_check(bank, rows, planes, layer_begin, layer_count, extent)) return e;
  return k_out && v_out ? EKV_OK : EKV_E_ARG;
}

int ekv_kv8_quantize(const ekv_bank* bank, const ekv_kv8* q8, int32_t dtype, int32_t layer_begin, int32_t layer_count, int32_t extent,
                     void* stream) {
  if (int e = quantize_check(bank, EKV_ROWS_kv8, ekv_planes(q8), dtype, layer_begin, layer_count, extent)) return e;
  drop_stale_error();
  return launch_code(ekv_launch_kv8_quantize(bank, q8, dtype == EKV_DTYPE_BF16, layer_begin, layer_count, extent, static_cast<hipStream_t>(stream)));
}

int ekv_kv8_dequantize(const ekv_bank* bank, const ekv_kv8* q8, int32_t out_dtype, int32_t layer_begin, int32_t layer_count,
                       int32_t extent, void* k_out, void* v_out, void* stream) {
  if (int e = dequantize_check(bank, EKV_ROWS_kv8, ekv_planes(q8), out_dtype, layer_begin, layer_count, extent, k_out, v_out)) return e;
  drop_stale_error();
  return launch_code(ekv_launch_kv8_dequantize(bank, q8, out_dtype, layer_begin, layer_count, extent, k_out, v_out, static_cast<hipStream_t>(stream)));
}

int ekv_kv4_quantize(const ekv_bank* bank, const ekv_kv4* q4, int32_t dtype, int32_t layer_begin, int32_t layer_count, int32_t extent,
                     void* stream) {
  if (int e = quantize_check(bank, EKV_ROWS_kv4, ekv_planes(q4), dtype, layer_begin, layer_count, extent)) return e;
  drop_stale_error();
  return launch_code(ekv_launch_kv4_quantize(bank, q4, dtype == EKV_DTYPE_BF16, layer_begin, layer_count, extent, static_cast<hipStream_t>(stream)));
}

int ekv_kv4_dequantize(const ekv_bank* bank, const ekv_kv4* q4, int32_t out_dtype, int32_t layer_begin, int32_t layer_count,
                       int32_t extent, void* k_out, void* v_out, void* stream) {
  if (int e = dequantize_check(bank, EKV_ROWS_kv4, ekv_planes(q4), out_dtype, layer_begin, layer_count, extent, k_out, v_out)) return e;
  drop_stale_error();
  return launch_code(ekv_launch_kv4_dequantize(bank, q4, out_dtype, layer_begin, layer_count, extent, k_out, v_out, static_cast<hipStream_t>(stream)));
}

int ekv_kv6_quantize(const ekv_bank* bank, const ekv_kv6* q6, int32_t dtype, int32_t layer_begin, int32_t layer_count, int32_t extent,
                     void* stream) {
  if (int e = quantize_check(bank, EKV_ROWS_kv6, ekv_planes(q6), dtype, layer_begin, layer_count, extent)) return e;
  drop_stale_error();
  return launch_code(ekv_launch_kv6_quantize(bank, q6, dtype == EKV_DTYPE_BF16, layer_begin, layer_count, extent, static_cast<hipStream_t>(stream)));
}

int ekv_kv6_dequantize(const ekv_bank* bank, const ekv_kv6* q6, int32_t out_dtype, int32_t layer_begin, int32_t layer_count,
                       int32_t extent, void* k_out, void* v_out, void* stream) {
  if (int e = dequantize_check(bank, EKV_ROWS_kv6, ekv_planes(q6), out_dtype, layer_begin, layer_count, extent, k_out, v_out)) return e;
  drop_stale_error();
  return launch_code(ekv_launch_kv6_dequantize(bank, q6, out_dtype, layer_begin, layer_count, extent, k_out, v_out, static_cast<hipStream_t>(stream)));
}

int ekv_kv84_quantize(const ekv_bank* bank, const ekv_kv84* q84, int32_t dtype, int32_t layer_begin, int32_t layer_count, int32_t extent,
                      void* stream) {
  if (int e = quantize_check(bank, EKV_ROWS_kv84, ekv_planes(q84), dtype, layer_begin, layer_count, extent)) return e;
  drop_stale_error();
  return launch_code(ekv_launch_kv84_quantize(bank, q84, dtype == EKV_DTYPE_BF16, layer_begin, layer_count, extent, static_cast<hipStream_t>(stream)));
}

int ekv_kv84_dequantize(const ekv_bank* bank, const ekv_kv84* q84, int32_t out_dtype, int32_t layer_begin, int32_t layer_count,
                        int32_t extent, void* k_out, void* v_out, void* stream) {
  if (int e = dequantize_check(bank, EKV_ROWS_kv84, ekv_planes(q84), out_dtype, layer_begin, layer_count, extent, k_out, v_out)) return e;
  drop_stale_error();
  return launch_code(ekv_launch_kv84_dequantize(bank, q84, out_dtype, layer_begin, layer_count, extent, k_out, v_out, static_cast<hipStream_t>(stream)));
}

int ekv_kv164_quantize(const ekv_bank* bank, const ekv_kv164* q164, int32_t dtype, int32_t layer_begin, int32_t layer_count, int32_t extent,
                       void* stream) {
  if (int e = quantize_check(bank, EKV_ROWS_kv164, ekv_planes(q164), dtype, layer_begin, layer_count, extent)) return e;
  drop_stale_error();
  return launch_code(ekv_launch_kv164_quantize(bank, q164, dtype == EKV_DTYPE_BF16, layer_begin, layer_count, extent, static_cast<hipStream_t>(stream)));
}

int ekv_kv164_dequantize(const ekv_bank* bank, const ekv_kv164* q164, int32_t out_dtype, int32_t layer_begin, int32_t layer_count,
                         int32_t extent, void* v_out, void* stream) {
  if (int e = dequantize_check(bank, EKV_ROWS_kv164, ekv_planes(q164), out_dtype, layer_begin, layer_count, extent, v_out, v_out)) return e;
  drop_stale_error();
  return launch_code(ekv_launch_kv164_dequantize(bank, q164, out_dtype, layer_begin, layer_count, extent, v_out, static_cast<hipStream_t>(stream)));
}

// ---- bank utilities: argument checks here, kernels and launch code in ekv_bank_ops.hip
int ekv_abi_version(void) { return EKV_ABI_VERSION; }

const char* ekv_strerror(int code) {
  switch (code) {
    case EKV_OK: return "ok";
    case EKV_E_ARG: return "invalid argument (null pointer or inconsistent sizes)";
    case EKV_E_UNSUPPORTED: return "unsupported shape (head_dim, group size, q_len or row width)";
    case EKV_E_WORKSPACE: return "workspace too small";
    case EKV_E_LAUNCH: return "kernel launch failed";
    default: return "unknown error";
  }
}

int ekv_bank_reset(const ekv_bank* bank, void* stream) {
  if (int e = check_bank(bank)) return e;
  drop_stale_error();
  return launch_code(ekv_launch_bank_reset(bank, static_cast<hipStream_t>(stream)));
}

int ekv_state_init(const ekv_bank* bank, int32_t layer_begin, int32_t layer_count, int32_t width, int32_t mode,
                   int32_t stride, void* stream) {
  if (int e = check_bank(bank)) return e;
  if (int e = check_layers(bank, layer_begin, layer_count)) return e;
  if (!bank->score_sum || !bank->score_sq || !bank->score_cnt || width < 0 || width > bank->cap || mode < 0 || mode > 2)
    return EKV_E_ARG;
  drop_stale_error();
  return launch_code(ekv_launch_state_init(bank, layer_begin, layer_count, width, mode, stride, static_cast<hipStream_t>(stream)));
}

int ekv_gather_ordered(const ekv_bank* bank, int32_t layer_begin, int32_t layer_count, int32_t n_slots, void* k_out,
                       void* v_out, void* stream) {
  if (int e = check_bank(bank)) return e;
  if (int e = check_layers(bank, layer_begin, layer_count)) return e;
  if (!k_out || !v_out || n_slots < 0 || n_slots > bank->cap) return EKV_E_ARG;
  if (n_slots == 0) return EKV_OK;
  drop_stale_error();
  return launch_code(ekv_launch_rows_copy(bank, true, layer_begin, layer_count, 0, n_slots, k_out, v_out, static_cast<hipStream_t>(stream)));
}

int ekv_scatter_rows(const ekv_bank* bank, int32_t layer_begin, int32_t layer_count, int32_t pos_begin, int32_t n,
                     const void* k_in, const void* v_in, void* stream) {
  if (int e = check_bank(bank)) return e;
  if (int e = check_layers(bank, layer_begin, layer_count)) return e;
  if (!k_in || !v_in || pos_begin < 0 || n < 0 || pos_begin + n > bank->cap) return EKV_E_ARG;
  if (n == 0) return EKV_OK;
  drop_stale_error();
  return launch_code(ekv_launch_rows_copy(bank, false, layer_begin, layer_count, pos_begin, n, const_cast<void*>(k_in), const_cast<void*>(v_in),
                                          static_cast<hipStream_t>(stream)));
}

// (both conversions stage four rows of words per head in LDS: n_slots wide to the slot layout, cap wide back)
static int rows_convert_check(const ekv_bank* bank, int32_t layer_begin, int32_t layer_count, int32_t n_slots, size_t lds) {
  if (int e = check_bank(bank)) return e;
  if (int e = check_layers(bank, layer_begin, layer_count)) return e;
  if (!bank->score_sum || !bank->birth || !bank->slot_state || n_slots < 0 || n_slots > bank->cap) return EKV_E_ARG;
  return lds > 150 * 1024 ? EKV_E_UNSUPPORTED : EKV_OK;
}

int ekv_rows_to_slots(const ekv_bank* bank, int32_t layer_begin, int32_t layer_count, int32_t n_slots, void* stream) {
  const size_t lds = (size_t)4 * n_slots * 4;
  if (int e = rows_convert_check(bank, layer_begin, layer_count, n_slots, lds)) return e;
  drop_stale_error();
  return launch_code(ekv_launch_rows_to_slots(bank, layer_begin, layer_count, n_slots, lds, static_cast<hipStream_t>(stream)));
}

int ekv_rows_to_order(const ekv_bank* bank, int32_t layer_begin, int32_t layer_count, int32_t n_slots, void* stream) {
  const size_t lds = bank ? (size_t)4 * bank->cap * 4 : 0;
  if (int e = rows_convert_check(bank, layer_begin, layer_count, n_slots, lds)) return e;
  drop_stale_error();
  return launch_code(ekv_launch_rows_to_order(bank, layer_begin, layer_count, n_slots, lds, static_cast<hipStream_t>(stream)));
}

int ekv_compact_inplace(const ekv_bank* bank, int32_t layer_begin, int32_t layer_count, int32_t n_slots, int32_t n_evict,
                        const int32_t* evict_ids, void* stream) {
  if (int e = check_bank(bank)) return e;
  if (int e = check_layers(bank, layer_begin, layer_count)) return e;
  if (!evict_ids || n_evict <= 0 || n_evict >= n_slots || n_slots > bank->cap) return EKV_E_ARG;
  drop_stale_error();
  return launch_code(ekv_launch_compact_inplace(bank, layer_begin, layer_count, n_slots, n_evict, evict_ids, static_cast<hipStream_t>(stream)));
}

}  // extern "C"
