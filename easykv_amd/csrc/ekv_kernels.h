// Internal launch interface between the C ABI (ekv_abi.hip) and the kernels; what the planner (ekv_plan.h) decides travels in EkvStepPlan.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "../../include/easykv_hip.h"
#include "ekv_geometry.h"

// The row format of a bank's K/V rows: the `rows` word of a manifest line (ekv_instances.def), and what a call of the step family says
// about its bank.  kv16: 16-bit rows.  kv8: FP8 codes + fp32 row scales (ekv_kv8).  kv4: MXFP4 codes + E8M0 block exponents (ekv_kv4).
// kv6: MXFP6 (e2m3) codes + E8M0 block exponents (ekv_kv6).  kv84: FP8 K codes + fp32 row scales, MXFP4 V codes + E8M0 block exponents (ekv_kv84).
// kv164: the bank's 16-bit K rows, MXFP4 V codes + E8M0 block exponents (ekv_kv164).
enum EkvRows : int32_t { EKV_ROWS_kv16, EKV_ROWS_kv8, EKV_ROWS_kv4, EKV_ROWS_kv6, EKV_ROWS_kv84, EKV_ROWS_kv164 };

// The resident rows of a one-launch decode step as they travel in EkvAttnArgs.fused_order / EkvStepPlan.fused_order (bits 16-23)
#define EKV_RESIDENT_UNIT 32      // rows of one wave iteration of the stream (EkvDecodeGeom::RW at head_dim 128)
#define EKV_RESIDENT_BITS(rows) ((((rows) / EKV_RESIDENT_UNIT) > 255 ? 255 : ((rows) / EKV_RESIDENT_UNIT)) << 16)
#define EKV_RESIDENT_ROWS(order) ((((order) >> 16) & 255) * EKV_RESIDENT_UNIT)
// Rule source 3 of the mixed phase order (bits 4-5 of fused_order = 3; the 8-wave flagship instances): order K for the workgroups at or
// past a threshold in the grid's dispatch order (layer-major, head-minor).  The threshold travels in the rule's mask (bits 8-11, high
// nibble) and bound (bits 12-15, low nibble) fields, in units of 8 workgroups: 0 .. 2040.
#define EKV_ORDER_ROUND_UNIT 8
#define EKV_ORDER_ROUND_BITS(wgs) \
  (((((wgs) / EKV_ORDER_ROUND_UNIT > 255 ? 255 : (wgs) / EKV_ORDER_ROUND_UNIT) >> 4) << 8) | ((((wgs) / EKV_ORDER_ROUND_UNIT > 255 ? 255 : (wgs) / EKV_ORDER_ROUND_UNIT) & 15) << 12))
#define EKV_ORDER_ROUND_THRESHOLD(order) ((((((order) >> 8) & 15) << 4) | (((order) >> 12) & 15)) * EKV_ORDER_ROUND_UNIT)

// One kernel launch sequence entry of a step (EkvStepPlan::list), in issue order.
enum EkvLaunchKind : int32_t {
  EKV_RUN_FUSED_DECODE,   // ekv_launch_decode_fused: the whole decode step
  EKV_RUN_CHUNK_LDS,      // ekv_launch_chunk_lds: the whole small-row chunk step
  EKV_RUN_RESIDENT,       // ekv_launch_attn_resident: the whole logits-resident chunk step
  EKV_RUN_DECODE,         // ekv_launch_attn_decode: split decode attention
  EKV_RUN_CHUNK,          // ekv_launch_attn_chunk
  EKV_RUN_FLUSH,          // ekv_launch_attn_chunk: the deferred column-sum pass of all layers, from the kept queries
  EKV_RUN_FOLD, EKV_RUN_RANGE, EKV_RUN_DECODE_SCORE, EKV_RUN_TOVA_MEAN, EKV_RUN_SCORE_SELECT,
  EKV_RUN_LONG_FOLD,      // ekv_launch_long_fold: the fold of a long call whose generic scorer would have folded the output itself
  EKV_RUN_LONG_SCORE      // ekv_launch_score_long: sweep + select of the long-row scorer (two kernels) where the plain plan has EKV_RUN_SCORE_SELECT
};
struct EkvLaunch {
  int32_t kind, kernel_count;
  int32_t skip_fold;   // EkvScoreArgs.skip_fold of this launch
  int32_t passes;      // EKV_RUN_CHUNK / _FLUSH: pass bits of ekv_launch_attn_chunk
  int32_t fuse, tail;  // ... the scorer runs as the tail of the 16x16 one-pass kernel / of the wide column-sum pass
};

// Everything ekv_step_attend decides about a step, from the bank and step descriptors alone (resolve_call, ekv_plan.cpp): nothing is
// dereferenced.  ekv_step_attend, ekv_step_check, ekv_step_plan, ekv_step_info and ekv_workspace_bytes — and their kv8 / batch kin — all read it.
struct EkvStepPlan {
  int32_t t_pad, n_split, rows_per_split;
  int32_t n_partials;   // partials per query row the scorer folds (chunk kernels emit 2 per split)
  int32_t qb_rows, n_qblocks, n_col_parts;
  int32_t fused_nw;     // waves per workgroup of the fused decode kernel for this launch (4 or 8)
  int32_t fused_order;  // phase order of its workgroups (ekv_decode_fused_order)
  int32_t l_pad, phys_extent;   // see EkvAttnArgs
  int32_t two_pass;
  int32_t wide;             // chunk step on the wide-query-block kernel (ekv_attn_wide.inc): ONE partial per split, ONE column-sum row
  int32_t resident;         // whole scored chunk step on the logits-resident kernel (ekv_attn_resident.inc): one launch, unsplit
  int32_t fold_in_kernel;   // chunk step whose attention kernel writes the final output itself (no partials, no fold)
  int32_t fold_in_decode;   // split decode step whose last-arriving split of a head folds the partials (ekv_bank.arrive)
  int32_t flush_unsplit;    // deferred flush: the column-sum pass runs unsplit over the one pass's key-range statistics
  int32_t slot_rows, slot_tail_ok;   // fused decode step on the slot-indexed score rows (EKV_PHASE_SLOT_ROWS / _TAIL_OK)
  int32_t bf16;             // 16-bit tensors are bf16: the launches run the EKV_BF16 kernel instances
  int32_t rows;             // EkvRows of the bank's K/V rows: the decode launches run the instances of that row format
  int32_t batch;            // a batched decode step (an ekv_seq call): the plan of the envelope; the launches run the batch instances
  int32_t strides[6];       // q, kv, out row strides (token, head) in elements, the dense layout filled in
  // Workspace: byte offsets of this call's slices (a deferred call's layout spans every deferred layer), -1 = not in the layout
  int64_t logits;     // [layer_count][Hq][q_len][t_pad]   raw q.k/sm_div of every live position
  int64_t partials;   // [layer_count][Hq][q_len][n_partials][D+2]   (m, l, o[D]) per key-range split
  int64_t tova_row;   // [layer_count][t_pad]   head-averaged last-query row (tova_head_mean)
  int64_t big_rows;   // [layer_count][H][3][t_pad] working copies of the score rows when they exceed one CU's LDS
  int64_t stats, colsum, row_stats;   // see EkvAttnArgs
  int64_t q_keep;     // deferred wide two-pass chunk steps: [layer_count][Hq][q_len][D] raw queries kept for the flush's column-sum pass
  int64_t q_rot;      // rope_on_read chunk steps on the 16x16 kernel: [2][layer_count][Hq][q_len][D] rotated queries, fp16 hi then lo
  size_t bytes;       // workspace the call needs
  int32_t one_launch;   // the whole step is ONE launch
  int32_t n_launches;   // kernel launches of the call: the sum of list[].kernel_count
  int32_t n_list;
  EkvLaunch list[6];
  // long calls (ekv_long_*, ekv_plan.cpp "long rows"): the step ends in the long-row scorer; column tiles per head of its sweep; byte
  // offset of its selection keys [layer_count][H][t_pad] uint32 (-1 = not in the layout)
  int32_t long_rows, long_tiles;
  int64_t key_rows;
  int32_t capped;       // an ekv_cap_* call: the launches run the EKV_SOFTCAP instances (chunk steps: the one-tile 16x16x32 build alone)
  int32_t sink;         // an ekv_sink_* call: the launches run the EKV_SINK instances (chunk steps likewise; decode steps in phase order F, no resident rows)
  int32_t window;       // an ekv_win_* call: the launches run the EKV_WINDOW instances (with sinks: the EKV_SINK + EKV_WINDOW ones); planned as the sink call
  int32_t pooled;       // an ekv_pool_* call: EKV_RUN_SCORE_SELECT runs the EKV_POOL instances of the generic scorer; every in-kernel scorer tail is off
  // adaptive calls (ekv_ada_*, ekv_plan.cpp "adaptive head budgets"): planned as the pooled call; EKV_RUN_SCORE_SELECT runs rank + allot +
  // select (three kernels).  Byte offsets of the exported ranking keys [layer_count][H][t_pad] uint32 and of the class bytes
  // [layer_count][H][t_pad] uint8 (0 forced, 1 free, 2 neither), behind everything the pooled layout holds (-1 = not in the layout)
  int32_t adaptive;
  int64_t ada_keys, ada_cls;
  int32_t heads;        // an ekv_heads_* call: the plan of the envelope; EKV_RUN_DECODE / EKV_RUN_DECODE_SCORE run the EKV_HEADS instances
};
// The table of a batched decode step as the kernels' batch instances receive it: BY VALUE, behind the argument structs of the uniform
// kernel (2304 bytes of the 4 KB a launch may carry).  Workgroup (head, entry ll) shadows the per-step fields of its argument structs
// from e[ll] with wave-uniform loads before anything else; nothing is staged in device memory and no copy precedes the launch.
struct EkvSeqTable {
  ekv_seq e[EKV_MAX_SEQS];      // phys_extent resolved (resolve_call)
};

// The __half* members below point at 16-bit rows: fp16, or bf16 for the EKV_BF16 kernel instances (ekv_common.h: rows move as
// bytes, and every element access of a kernel goes through ekv_e / ekv_h8 / ekv_to_e).
struct EkvAttnArgs {
  const __half* k;
  const __half* v;
  __half* k_w;  // same buffers, writable (append of the new rows)
  __half* v_w;
  const int32_t* slot_of_pos;
  const __half* q;
  const __half* k_new;
  const __half* v_new;
  float* logits;
  float* partials;
  const float* rope_cos;
  const float* rope_sin;
  __half* q_rot_hi;  // chunk kernels with rope_on_read: queries rotated by ekv_rope_q_kernel (hi + lo fp16 pair)
  __half* q_rot_lo;
  float* row_stats;    // with out_direct, one-pass scored steps: [layer_count][Hq][q_len][2] final (max, sum exp) per query row
  __half* out_direct;  // chunk kernels, unsplit heads: fold the two key halves in the kernel and write the fp16 output here
  // FP8 rows (ekv_kv8_step_attend; the decode kernels' kv8 instances only — decode steps have no use for `stats` / `colsum`, whose
  // storage the two pointers share, so the struct and with it every 16-bit kernel instance stays as it was): k / v / k_w / v_w are the
  // code planes, one byte per element, and k_scale / v_scale the fp32 row scales [n_layers][H][cap] at the rows' physical indices
  // MXFP4 rows (ekv_kv4_step_attend; the kv4 instances only), likewise: k / v / k_w / v_w are the code planes, two codes per byte, and
  // k_exp / v_exp the E8M0 bytes [n_layers][H][cap][head_dim / 32].  MXFP6 rows (the kv6 instances): the same with 24-byte blocks of 32 codes
  // FP8 keys with MXFP4 values (the kv84 instances): k / k_w / k_scale as for FP8 rows, v / v_w / v_exp as for MXFP4 rows
  // 16-bit keys with MXFP4 values (the kv164 instances): k / k_w are the bank's 16-bit K rows, v / v_w / v_exp as for MXFP4 rows
  union {
    float* stats;      // two-pass chunk steps: [layer_count][Hq][q_len][2*n_split][2] (max, sum exp) per key-range half split
    float* k_scale;
    uint8_t* k_exp;
  };
  union {
    float* colsum;     // two-pass chunk steps: [layer_count][H][n_col_parts][2][t_pad] column sums of pbar and pbar^2
    float* v_scale;
    uint8_t* v_exp;
  };
  int32_t n_col_parts;   // = query-tile waves per workgroup (2 or 4) * n_qblocks
  int32_t n_q_heads, n_kv_heads, cap, n_slots, q_len, n_split, rows_per_split, t_pad, layer_begin, causal;
  int32_t qb_rows, n_qblocks;  // chunk kernels: queries per query block, number of query blocks
  int32_t phys_extent;         // fused decode step, physical-order stream: live rows have physical index < phys_extent
  int32_t l_pad;               // fused decode step: pitch of a logits row in LDS (t_pad, or align(phys_extent, 64))
  uint32_t* arrive;            // split decode kernel: non-null = fold the key-range partials in the kernel (last-arriving split of a
                               //   head) and write the fp16 output to out_direct; the bank's counters [n_layers][H], 0 when idle
  float sm_div;
  // soft-capped logits (the ekv_cap_* calls; read by the EKV_SOFTCAP instances only): the cap, finite and > 0.  It fills the padding
  // behind sm_div, so the struct, its offsets and with them every other instance stay as they were.
  float softcap;
  // deferred column-sum pass of the wide-block kernel (ekv_step.defer_layers, chunk steps): the one pass of a layer keeps its raw
  // queries in q_keep ([layers][Hq][q_len][D], this call's slice); the column-sum pass at the flush reads them as `q` and takes the
  // chunk's own K rows from the cache slots (new_in_cache) instead of k_new
  __half* q_keep;
  int32_t new_in_cache;
  // column-sum pass of the wide-block kernel: 1 = the scorer of the step runs as the tail of this launch (ekv_wide_tail.h; the
  // EkvScoreArgs are the launch's second argument); set only for heads whose column sums ONE workgroup writes
  // fused decode step: the phase order of its workgroups (ekv_decode_fused_order; 0 = every workgroup streams K+V and then runs its
  // tail).  Decode steps have no use for score_tail, whose storage it shares, so the struct stays as it was.
  // Bits 16-23 of fused_order: the planned resident rows of the launch in units of 32 rows (EKV_RESIDENT_ROWS; ekv_decode_resident_rows,
  // ekv_plan.h) — physical rows below it are read with default-policy loads, the rest non-temporally.  Only the 16-bit slot-indexed
  // head_dim 128 instances of GQA factor 1 read the bits.
  union {
    int32_t score_tail;
    int32_t fused_order;
  };
  // row strides in elements (ekv_step.*_stride, ABI 8; always filled in: the dense layout is q_ts = D, q_hs = q_len * D, ...): row
  // (layer ll, head hd, token i) of q sits at ((size_t)ll * n_q_heads * q_len) * D + hd * q_hs + i * q_ts, k_new / v_new and out alike
  int32_t q_ts, q_hs, kv_ts, kv_hs, o_ts, o_hs;
  int32_t n_stat_parts;     // column-sum pass: (max, sum) partials per query row in `stats` when that differs from this launch's n_split (0 = n_split)
};

struct EkvScoreArgs {
  int32_t* slot_of_pos;
  float* score_sum;
  float* score_sq;
  float* score_cnt;
  const float* logits;
  const float* partials;
  const float* colsum;   // non-null: column sums from the two-pass chunk kernel replace the logits
  float* big_rows;       // non-null: score rows wider than one CU's LDS — the scorer keeps its working copies of S / Q / C in this
  int big_stride;        //   scratch ([layer_count][H][3][big_stride] floats) and only the selection keys in LDS
  const float* row_stats;   // non-null: final row statistics written by the chunk kernel (its in-kernel fold)
  int32_t n_col_parts;
  float* tova_row;
  __half* out;
  int32_t* evict_ids;
  int32_t n_q_heads, n_kv_heads, head_dim, cap, n_slots, q_len, n_split, t_pad, layer_begin;
  int32_t score_off, policy, accumulate, n_evict, win_lo, win_tail, roco_k1, roco_tail, range_start, tova_head_mean,
      causal;
  float count_add, count_tail_step;
  int32_t skip_fold;   // 1: the attention output was already folded by ekv_fold_kernel (scorer off the critical path)
  int32_t o_ts, o_hs;  // row strides of `out` in elements (see EkvAttnArgs)
  // slot-indexed score rows (ekv_step.phases & EKV_PHASE_SLOT_ROWS, fused decode step; ekv_decode_tail.h): score_sum / score_sq /
  // score_cnt are indexed by physical row, score_cnt holds the count base, birth[row] the order key, slot_state[head] = (g, next birth, threshold hint of the decode step, threshold hint of the chunk_lds kernel — the hints in any layout)
  int32_t* birth;
  float* slot_state;
  float* cnt_tail;        // parked tail of the ordered count row (second half of ekv_bank.birth)
  int32_t slot_tail_ok;   // EKV_PHASE_SLOT_TAIL_OK: the newest `tail` entries are known to have consecutive births
};

// bf16 (the launchers below that take it): run the EKV_BF16 instances — 16-bit rows of q, k_new, v_new, out and the bank read and
// written as bf16 (ekv_common.h); the planner never sends a RoPE-on-read step there.
// tb (the decode launchers): NULL = a uniform step of `count` layers; the table of a batched decode step = the batch instances (16-bit
// or FP8 rows, plain keys, ordered score rows): `a` / `sc` are the envelope's arguments with layer_begin = 0 and a.arrive = the bank's
// counters, and `count` is the number of table entries, one workgroup row each.
// rows: the instances of that row format (kv8: a.k_scale / a.v_scale set, kv4 / kv6: a.k_exp / a.v_exp, kv84: a.k_scale / a.v_exp, kv164: a.v_exp; plain keys either way)
// capped (every launcher below that takes it): the EKV_SOFTCAP instances, a.softcap set (ekv_cap_* calls)
hipError_t ekv_launch_attn_decode(const EkvAttnArgs& a, const EkvSeqTable* tb, int head_dim, int count, hipStream_t s, bool bf16, EkvRows rows,
                                  bool capped = false);
// passes (wide-block kernel, two-pass scheme): bit 0 = the one pass (output + row statistics), bit 1 = the column-sum pass
// tail_sc (wide-block kernel, two passes, passes & 2): the step's scorer runs as the tail of the column-sum pass (ekv_wide_tail.h)
// wide: the wide-block kernel (ekv_chunk_wide, ekv_plan.h)
hipError_t ekv_launch_attn_chunk(const EkvAttnArgs& a, int head_dim, int layer_count, bool wide, bool two_pass, hipStream_t s,
                                 const EkvScoreArgs* fuse_sc, int passes, const EkvScoreArgs* tail_sc, bool bf16, bool capped = false);
hipError_t ekv_launch_attn_resident(const EkvAttnArgs& a, const EkvScoreArgs& sc, int layer_count, hipStream_t s, bool bf16);
hipError_t ekv_launch_tova_headmean(const EkvScoreArgs& a, int layer_count, hipStream_t s);
hipError_t ekv_launch_score_select(const EkvScoreArgs& a, int layer_count, hipStream_t s, bool bf16);
hipError_t ekv_launch_decode_fused(const EkvAttnArgs& a, const EkvScoreArgs& sc, const EkvSeqTable* tb, int head_dim, int count, int nw,
                                   hipStream_t s, bool bf16, EkvRows rows, bool capped = false);
// Pooled selection (the ekv_pool_* calls; the EKV_POOL instances of ekv_score_select.inc): what the pooled scorer receives as its last
// argument — the radius r >= 1 (kernel size 2r + 1) and the op (EKV_POOL_MAX / EKV_POOL_AVG) — and its launcher: the 512-thread build, or
// the 1024-thread one where the unpooled dispatch would pick it (rows in scratch, one workgroup per CU).
struct EkvPoolArgs {
  int32_t radius, op;
};
hipError_t ekv_launch_score_select_pool(const EkvScoreArgs& a, const EkvPoolArgs& pool, int layer_count, hipStream_t s, bool bf16);
// Adaptive head budgets (the ekv_ada_* calls; include/easykv_hip.h): what the EKV_ADA instances of ekv_score_select.inc and the allot kernel
// (ekv_score_allot.inc) receive as their last argument.  phase 0 = rank: accumulate, write the score rows back, pool, export the W ranking
// keys of the head and its class bytes.  phase 1 = select: read the score rows and the keys back, k = k_out[ll][h], then the scorer's own
// marking, scan, write-back and compaction.  keys / cls: this launch's slices, rows `stride` elements apart, [layer_count][H][stride].
// k_out: device int32 [layer_count][H], written by the allot kernel between the two (one workgroup per layer).
struct EkvAdaArgs {
  int32_t radius, op, evict_min, evict_max;
  int32_t phase, stride;
  uint32_t* keys;
  uint8_t* cls;
  int32_t* k_out;
};
hipError_t ekv_launch_score_select_ada(const EkvScoreArgs& a, const EkvAdaArgs& ada, int layer_count, hipStream_t s, bool bf16);
hipError_t ekv_launch_score_allot(const EkvScoreArgs& a, const EkvAdaArgs& ada, int layer_count, hipStream_t s);
// Attention sinks (the ekv_sink_* calls; EKV_SINK instances, ekv_common.h): the launchers of a sink step.  sinks: device fp32
// [bank->n_layers][n_q_heads], indexed by bank layer.  16-bit rows, plain keys, one sequence; head_dim 64 / 128.  The chunk launcher runs
// the 16x16x32 kernel in its one-tile build (pass: 0 one pass, 1 statistics pass, 2 exact pass; fuse_sc: the scorer as the one pass's tail).
hipError_t ekv_launch_attn_decode_sink(const EkvAttnArgs& a, const float* sinks, int head_dim, int count, hipStream_t s, bool bf16);
hipError_t ekv_launch_decode_fused_sink(const EkvAttnArgs& a, const EkvScoreArgs& sc, const float* sinks, int head_dim, int count, int nw,
                                        hipStream_t s, bool bf16);
hipError_t ekv_launch_decode_score_sink(const EkvScoreArgs& sc, const float* sinks, int count, hipStream_t s, bool bf16);
hipError_t ekv_launch_tova_headmean_sink(const EkvScoreArgs& a, const float* sinks, int layer_count, hipStream_t s);      // (ekv_score_select.inc, EKV_SINK build)
hipError_t ekv_launch_attn_chunk_sink(const EkvAttnArgs& a, const float* sinks, int head_dim, int layer_count, bool two_pass, hipStream_t s,
                                      const EkvScoreArgs* fuse_sc, bool bf16);
// Sliding windows (the ekv_win_* calls; EKV_WINDOW instances, ekv_common.h): what the window kernels receive as their last argument, and
// the launchers of a window step.  tok_pos: int32 [bank->n_layers][n_kv_heads][cap], indexed by physical row, written by the kernel that
// appends a row (the decode stream's and the chunk kernel's append sites: row i of the step is at q_pos0 + i); windows: int32 [bank->n_layers], 0 = no window.
// sinks == NULL runs the window-alone instances (head_dim 128), sinks != NULL the sink + window ones (head_dim 64).
struct EkvWinArgs {
  int32_t* tok_pos;
  const int32_t* windows;
  int32_t q_pos0;      // token position of the step's (first) query row
};
hipError_t ekv_launch_attn_decode_win(const EkvAttnArgs& a, const float* sinks, const EkvWinArgs& win, int head_dim, int count, hipStream_t s, bool bf16);
hipError_t ekv_launch_decode_fused_win(const EkvAttnArgs& a, const EkvScoreArgs& sc, const float* sinks, const EkvWinArgs& win, int head_dim, int count,
                                       int nw, hipStream_t s, bool bf16);
// The chunk launcher runs the 16x16x32 kernel's window instances in the one-tile build, as ekv_launch_attn_chunk_sink runs the sink ones.
hipError_t ekv_launch_attn_chunk_win(const EkvAttnArgs& a, const float* sinks, const EkvWinArgs& win, int head_dim, int layer_count, bool two_pass,
                                     hipStream_t s, const EkvScoreArgs* fuse_sc, bool bf16);
// (the scorer behind the split kernel reads exported logits and partials, never a K/V row or a position: a window step runs the plain
// scorer instance, a sink + window step the sink one)
// ekv_softcap_eval: out[i] = ekv_softcap(x[i] / sm_div, cap) (ekv_attn_decode_dispatch.hip)
hipError_t ekv_launch_softcap_eval(const float* x, int64_t n, float sm_div, float cap, float* out, hipStream_t s);
// Long-row scorer (ekv_score_long.inc; one build for fp16 and bf16 banks).  a.big_rows and key_rows ([layer_count][H][a.big_stride]
// uint32) must be set.  plain_big: the plain call's plan of this step keeps its rows in scratch (it decides which build of the generic
// scorer the plain call runs, and with it the batch width of the partials fold: ekv_score_select_threads).
hipError_t ekv_launch_score_long(const EkvScoreArgs& a, uint32_t* key_rows, bool plain_big, int layer_count, hipStream_t s);
hipError_t ekv_launch_long_fold(const EkvScoreArgs& a, bool plain_big, int layer_count, hipStream_t s, bool bf16);
// What workgroup (head, entry z) of a batch instance does first: its argument structs are the envelope's with the per-step fields
// replaced by its entry's (scalar loads from the kernel arguments).  layer_begin = layer - z: every `layer_begin + ll` of the kernel
// body then names the entry's bank layer, while the workspace and the call's tensors stay indexed by ll = z.
__device__ __forceinline__ EkvAttnArgs ekv_batch_attn_args(const EkvAttnArgs& env, const ekv_seq& e, int z) {
  EkvAttnArgs a = env;
  a.n_slots = e.n_slots;
  a.phys_extent = e.phys_extent;
  a.layer_begin = e.layer - z;
  return a;
}
__device__ __forceinline__ EkvScoreArgs ekv_batch_score_args(const EkvScoreArgs& env, const ekv_seq& e, int z) {
  EkvScoreArgs sc = env;
  sc.n_slots = e.n_slots;
  sc.layer_begin = e.layer - z;
  sc.score_off = e.score_off;
  sc.n_evict = e.n_evict;
  sc.win_lo = e.win_lo;
  sc.win_tail = e.win_tail;
  sc.roco_k1 = e.roco_k1;
  sc.range_start = e.range_start;
  return sc;
}
// What the heads instances (EKV_HEADS = 1, below) receive as their last argument: the device table of ekv_heads and its growth.
struct EkvHeadsArgs {
  const int32_t* rows;      // device int32 [bank->n_layers][n_kv_heads]
  int32_t grow;
};
// What workgroup (head h, layer z) of a heads instance does first: T = rows[layer][h] + grow + 1 replaces the envelope's n_slots.  Every
// other field, the pitches among them (t_pad, l_pad, n_split, rows_per_split), stays the envelope's; everything a kernel derives from
// n_slots it derives from its own copy.
__device__ __forceinline__ EkvAttnArgs ekv_heads_attn_args(const EkvAttnArgs& env, const EkvHeadsArgs& hd, int h, int z) {
  EkvAttnArgs a = env;
  a.n_slots = hd.rows[(size_t)(env.layer_begin + z) * env.n_kv_heads + h] + hd.grow + 1;
  return a;
}
__device__ __forceinline__ EkvScoreArgs ekv_heads_score_args(const EkvScoreArgs& env, const EkvHeadsArgs& hd, int h, int z) {
  EkvScoreArgs sc = env;
  sc.n_slots = hd.rows[(size_t)(env.layer_begin + z) * env.n_kv_heads + h] + hd.grow + 1;
  return sc;
}
#if defined(EKV_HEADS) && EKV_HEADS
#define EKV_HEADS_ONLY(...) __VA_ARGS__
#else
#define EKV_HEADS_ONLY(...)
#endif
// How a kernel source spells its batch instance (EKV_BATCH = 1, set for the batch lines of ekv_instances.def before anything is
// included; off, the macros vanish and the source is the uniform kernel's, token for token): the argument structs arrive under the
// names a_env / sc_env with the table behind them, and EKV_SHADOW_* declares `a` / `sc` as this workgroup's own copies.
// EKV_TB_DEREF: what a host launcher (which always takes the table's address) hands to the launch templates.
#if defined(EKV_BATCH) && EKV_BATCH
#define EKV_BATCHING batch
#define EKV_BATCH_TAG _batch
#define EKV_ARG_A a_env
#define EKV_ARG_SC sc_env
#define EKV_TB_PARAM , const EkvSeqTable tb
#define EKV_TB_DECL , const EkvSeqTable& tb
#define EKV_TB_PASS , tb
#define EKV_TB_DEREF , *tb
#define EKV_ARRIVE_ROW(ll) (a.layer_begin + (ll))      // the arrival counters are the bank's: indexed by the entry's layer
#define EKV_SHADOW_A(z) const EkvAttnArgs a = ekv_batch_attn_args(a_env, tb.e[z], (int)(z));
#define EKV_SHADOW_SC(z) const EkvScoreArgs sc = ekv_batch_score_args(sc_env, tb.e[z], (int)(z));
#elif defined(EKV_HEADS) && EKV_HEADS
// The third spelling (EKV_HEADS = 1, the EKV_*_HEADS lines of the manifest): decode steps over KV heads of different lengths
// (include/easykv_hip.h, ekv_heads).  Nothing travels by value but a pointer and a word: EkvHeadsArgs is the LAST kernel argument, spelled
// through EKV_HEADS_ONLY like the sinks and the window struct, and workgroup (head, layer z) shadows n_slots of its argument structs with
// rows[layer_begin + z][head] + grow + 1 (one scalar load) before anything else.  The grid is the uniform kernel's, the layers are the
// call's own (no one-head view), the arrival counters are indexed as in the uniform kernel.  A source names its head index, EKV_HEAD_IDX,
// before its kernels (blockIdx.y in the attention kernel, blockIdx.x in the scorer).
#define EKV_BATCHING heads
#define EKV_BATCH_TAG _heads
#define EKV_ARG_A a_env
#define EKV_ARG_SC sc_env
#define EKV_TB_PARAM
#define EKV_TB_DECL
#define EKV_TB_PASS
#define EKV_TB_DEREF
#define EKV_ARRIVE_ROW(ll) (ll)
#define EKV_SHADOW_A(z) const EkvAttnArgs a = ekv_heads_attn_args(a_env, heads, (int)(EKV_HEAD_IDX), (int)(z));
#define EKV_SHADOW_SC(z) const EkvScoreArgs sc = ekv_heads_score_args(sc_env, heads, (int)(EKV_HEAD_IDX), (int)(z));
#else
#define EKV_BATCHING single
#define EKV_BATCH_TAG
#define EKV_ARG_A a
#define EKV_ARG_SC sc
#define EKV_TB_PARAM
#define EKV_TB_DECL
#define EKV_TB_PASS
#define EKV_TB_DEREF
#define EKV_ARRIVE_ROW(ll) (ll)
#define EKV_SHADOW_A(z)
#define EKV_SHADOW_SC(z)
#endif
#if defined(EKV_KV8) && EKV_KV8
#define EKV_ROWS kv8
#define EKV_ROWS_TAG _kv8
#elif defined(EKV_KV4) && EKV_KV4
#define EKV_ROWS kv4
#define EKV_ROWS_TAG _kv4
#elif defined(EKV_KV6) && EKV_KV6
#define EKV_ROWS kv6
#define EKV_ROWS_TAG _kv6
#elif defined(EKV_KV84) && EKV_KV84
#define EKV_ROWS kv84
#define EKV_ROWS_TAG _kv84
#elif defined(EKV_KV164) && EKV_KV164
#define EKV_ROWS kv164
#define EKV_ROWS_TAG _kv164
#else
#define EKV_ROWS kv16
#define EKV_ROWS_TAG
#endif

// soft-capped logits (EKV_SOFTCAP = 1: the EKV_DECODE_CAP and EKV_CHUNK_CAP lines of the manifest; ekv_common.h)
#if defined(EKV_SOFTCAP) && EKV_SOFTCAP
#define EKV_CAP_TAG _cap
#else
#define EKV_CAP_TAG
#endif

// attention sinks (EKV_SINK = 1: the EKV_*_SINK lines of the manifest; ekv_common.h)
#if defined(EKV_WINDOW) && EKV_WINDOW == 2 && !defined(EKV_SINK)
#define EKV_SINK 1      // (the sink + window instances: ekv_common.h)
#endif
#if defined(EKV_SINK) && EKV_SINK
#define EKV_SINK_TAG _sink
#else
#define EKV_SINK_TAG
#endif

// sliding windows (EKV_WINDOW = 1: the EKV_*_WIN lines of the manifest; ekv_common.h)
#if defined(EKV_WINDOW) && EKV_WINDOW
#define EKV_WIN_TAG _win
#else
#define EKV_WIN_TAG
#endif

// ---- kernel instances (ekv_instances.def; DESIGN.md "kernel instances")
// Kernel symbol of an instance = the kernel's name + independent tags that default to empty: _batch, _kv8, _cap, _sink, _win, _bf16 (ekv_common.h).  A
// kernel source renames itself with  #define ekv_x_kernel EKV_KERNEL_NAME(ekv_x_kernel)  (profiles and traces know these names).
#define EKV_KERNEL_NAME_(base, b, r, c, k, w, t) base##b##r##c##k##w##t
#define EKV_KERNEL_NAME_X(base, b, r, c, k, w, t) EKV_KERNEL_NAME_(base, b, r, c, k, w, t)
#define EKV_KERNEL_NAME(base) EKV_KERNEL_NAME_X(base, EKV_BATCH_TAG, EKV_ROWS_TAG, EKV_CAP_TAG, EKV_SINK_TAG, EKV_WIN_TAG, EKV_DT_TAG)
// Launcher of an instance = the family's entry + every word of its manifest line, in the line's order.  The instance (which pastes
// its own switches: EKV_D, EKV_KEYS, EKV_ELEM, EKV_ROWS, EKV_BATCHING, ...) and the dispatch tables (which paste the manifest's words)
// both spell it through these macros.
#define EKV_FN_DECODE_(fn, d, keys, elem, rows, batching) fn##_d##d##_##keys##_##elem##_##rows##_##batching
#define EKV_FN_DECODE(fn, d, keys, elem, rows, batching) EKV_FN_DECODE_(fn, d, keys, elem, rows, batching)
#define EKV_FN_DECODE_SCORE_(fn, elem, batching) fn##_##elem##_##batching
#define EKV_FN_DECODE_SCORE(fn, elem, batching) EKV_FN_DECODE_SCORE_(fn, elem, batching)
#define EKV_FN_ELEM_(fn, elem) fn##_##elem
#define EKV_FN_ELEM(fn, elem) EKV_FN_ELEM_(fn, elem)
#define EKV_FN_CHUNK_(d, m, elem) ekv_launch_attn_chunk_d##d##_m##m##_##elem
#define EKV_FN_CHUNK(d, m, elem) EKV_FN_CHUNK_(d, m, elem)
#define EKV_FN_CHUNK_CAP_(d, m, elem) ekv_launch_attn_chunk_cap_d##d##_m##m##_##elem
#define EKV_FN_CHUNK_CAP(d, m, elem) EKV_FN_CHUNK_CAP_(d, m, elem)
#define EKV_FN_SINK_(fn, elem, d) fn##_sink_d##d##_##elem
#define EKV_FN_SINK(fn, elem, d) EKV_FN_SINK_(fn, elem, d)      // (EKV_DECODE_SINK; EKV_DECODE_SCORE_SINK names no head_dim)
#define EKV_FN_WIN_(fn, elem, d) fn##_win_d##d##_##elem
#define EKV_FN_WIN(fn, elem, d) EKV_FN_WIN_(fn, elem, d)      // (EKV_DECODE_WIN)
#define EKV_FN_HEADS_(fn, elem, d) fn##_heads_d##d##_##elem
#define EKV_FN_HEADS(fn, elem, d) EKV_FN_HEADS_(fn, elem, d)      // (EKV_DECODE_HEADS; EKV_DECODE_SCORE_HEADS names no head_dim)
#define EKV_FN_SINK_WIN_(fn, elem, d) fn##_sink_win_d##d##_##elem
#define EKV_FN_SINK_WIN(fn, elem, d) EKV_FN_SINK_WIN_(fn, elem, d)      // (EKV_DECODE_SINK_WIN)
#define EKV_FN_CHUNK_WIN_(d, m, elem) ekv_launch_attn_chunk_win_d##d##_m##m##_##elem
#define EKV_FN_CHUNK_WIN(d, m, elem) EKV_FN_CHUNK_WIN_(d, m, elem)
#define EKV_FN_CHUNK_SINK_WIN_(d, m, elem) ekv_launch_attn_chunk_sink_win_d##d##_m##m##_##elem
#define EKV_FN_CHUNK_SINK_WIN(d, m, elem) EKV_FN_CHUNK_SINK_WIN_(d, m, elem)
#define EKV_FN_CHUNK_SINK_(d, m, elem) ekv_launch_attn_chunk_sink_d##d##_m##m##_##elem
#define EKV_FN_CHUNK_SINK(d, m, elem) EKV_FN_CHUNK_SINK_(d, m, elem)
#define EKV_FN_WIDE_(d, m, keys, elem) ekv_launch_attn_wide_d##d##_m##m##_##keys##_##elem
#define EKV_FN_WIDE(d, m, keys, elem) EKV_FN_WIDE_(d, m, keys, elem)
#define EKV_FN_D_ELEM_(fn, d, elem) fn##_d##d##_##elem
#define EKV_FN_D_ELEM(fn, d, elem) EKV_FN_D_ELEM_(fn, d, elem)      // (EKV_CHUNK_LDS, EKV_RESIDENT)
#define EKV_FN_SCORE_SELECT_(nt, elem) ekv_launch_score_select_nt##nt##_##elem
#define EKV_FN_SCORE_SELECT(nt, elem) EKV_FN_SCORE_SELECT_(nt, elem)
#define EKV_FN_SCORE_SELECT_POOL_(nt, elem) ekv_launch_score_select_pool_nt##nt##_##elem
#define EKV_FN_SCORE_SELECT_POOL(nt, elem) EKV_FN_SCORE_SELECT_POOL_(nt, elem)
#define EKV_FN_SCORE_SELECT_ADA_(nt, elem) ekv_launch_score_select_ada_nt##nt##_##elem
#define EKV_FN_SCORE_SELECT_ADA(nt, elem) EKV_FN_SCORE_SELECT_ADA_(nt, elem)
// the manifest's words as the fields of a table entry: booleans, and EKV_ROWS_<rows> above
#define EKV_IS_plain false
#define EKV_IS_rope true
#define EKV_IS_cap false      // (`cap`, the keys word in the launcher names of the soft-capped decode instances: plain keys ...
#define EKV_CAPPED_plain false
#define EKV_CAPPED_rope false
#define EKV_CAPPED_cap true   //  ... and capped logits)
#define EKV_IS_f16 false
#define EKV_IS_bf16 true
#define EKV_IS_single false
#define EKV_IS_batch true
// FP8 bank conversion (ekv_kv8.hip).  src_bf16: the 16-bit rows are bf16; out_kind: 0 fp16, 1 bf16, 2 fp32
hipError_t ekv_launch_kv8_quantize(const ekv_bank* bank, const ekv_kv8* q8, bool src_bf16, int layer_begin, int layer_count, int extent,
                                   hipStream_t s);
hipError_t ekv_launch_kv8_dequantize(const ekv_bank* bank, const ekv_kv8* q8, int out_kind, int layer_begin, int layer_count, int extent,
                                     void* k_out, void* v_out, hipStream_t s);
// MXFP4 bank conversion (ekv_kv4.hip), same arguments
hipError_t ekv_launch_kv4_quantize(const ekv_bank* bank, const ekv_kv4* q4, bool src_bf16, int layer_begin, int layer_count, int extent,
                                   hipStream_t s);
hipError_t ekv_launch_kv4_dequantize(const ekv_bank* bank, const ekv_kv4* q4, int out_kind, int layer_begin, int layer_count, int extent,
                                     void* k_out, void* v_out, hipStream_t s);
// MXFP6 bank conversion (ekv_kv4.hip, the conversion unit of the MX block formats), same arguments
hipError_t ekv_launch_kv6_quantize(const ekv_bank* bank, const ekv_kv6* q6, bool src_bf16, int layer_begin, int layer_count, int extent,
                                   hipStream_t s);
hipError_t ekv_launch_kv6_dequantize(const ekv_bank* bank, const ekv_kv6* q6, int out_kind, int layer_begin, int layer_count, int extent,
                                     void* k_out, void* v_out, hipStream_t s);
// FP8-key / MXFP4-value bank conversion (ekv_kv4.hip), same arguments
hipError_t ekv_launch_kv84_quantize(const ekv_bank* bank, const ekv_kv84* q84, bool src_bf16, int layer_begin, int layer_count, int extent,
                                    hipStream_t s);
hipError_t ekv_launch_kv84_dequantize(const ekv_bank* bank, const ekv_kv84* q84, int out_kind, int layer_begin, int layer_count, int extent,
                                      void* k_out, void* v_out, hipStream_t s);
// 16-bit-key / MXFP4-value bank conversion (ekv_kv4.hip): the V planes only, K is neither read nor written
hipError_t ekv_launch_kv164_quantize(const ekv_bank* bank, const ekv_kv164* q164, bool src_bf16, int layer_begin, int layer_count, int extent,
                                     hipStream_t s);
hipError_t ekv_launch_kv164_dequantize(const ekv_bank* bank, const ekv_kv164* q164, int out_kind, int layer_begin, int layer_count, int extent,
                                       void* v_out, hipStream_t s);
hipError_t ekv_launch_decode_score(const EkvScoreArgs& sc, const EkvSeqTable* tb, int count, hipStream_t s, bool bf16);
// Heads (the ekv_heads_* calls; EKV_HEADS instances): the split decode kernel with its in-kernel fold, and the scorer behind it.  `a` / `sc`
// are the envelope's arguments of a uniform step of `count` layers.  16-bit rows, plain keys, every head_dim of the decode kernels.
hipError_t ekv_launch_attn_decode_heads(const EkvAttnArgs& a, const EkvHeadsArgs& hd, int head_dim, int count, hipStream_t s, bool bf16);
hipError_t ekv_launch_decode_score_heads(const EkvScoreArgs& sc, const EkvHeadsArgs& hd, int count, hipStream_t s, bool bf16);
hipError_t ekv_launch_fold(const EkvScoreArgs& sc, int layer_count, hipStream_t s, bool bf16);

// Small-row chunk step with the logits in LDS (ekv_chunk_lds.inc): whole step in one launch, K and V read once.
hipError_t ekv_launch_chunk_lds(const EkvAttnArgs& a, const EkvScoreArgs& sc, int head_dim, int layer_count, hipStream_t s, bool bf16);

// ---- bank utility kernels (ekv_bank_ops.hip); the entry points (ekv_abi.hip) have checked the arguments
hipError_t ekv_launch_bank_reset(const ekv_bank* bank, hipStream_t s);
hipError_t ekv_launch_state_init(const ekv_bank* bank, int layer_begin, int layer_count, int width, int mode, int stride, hipStream_t s);
// gather: the first n slots of the layers, in order, to dense k_lin / v_lin; else scatter n dense rows to positions pos_begin ..
hipError_t ekv_launch_rows_copy(const ekv_bank* bank, bool gather, int layer_begin, int layer_count, int pos_begin, int n, void* k_lin, void* v_lin,
                                hipStream_t s);
hipError_t ekv_launch_compact_inplace(const ekv_bank* bank, int layer_begin, int layer_count, int n_slots, int n_evict, const int32_t* evict_ids,
                                      hipStream_t s);
// EKV_POLICY_RANGE: tb != NULL = a batched decode step (the range of each entry from the table; `st` is its envelope)
hipError_t ekv_launch_range_evict(const ekv_bank* bank, const ekv_step* st, const EkvSeqTable* tb, int32_t* evict_ids, hipStream_t s);
hipError_t ekv_launch_rows_to_slots(const ekv_bank* bank, int layer_begin, int layer_count, int n_slots, size_t lds, hipStream_t s);
hipError_t ekv_launch_rows_to_order(const ekv_bank* bank, int layer_begin, int layer_count, int n_slots, size_t lds, hipStream_t s);
// second half of ekv_bank.birth: the parked tail of the ordered count row (float), same [layer][head][cap] indexing
inline float* ekv_cnt_tail(const ekv_bank* bank) {
  return reinterpret_cast<float*>(bank->birth + (size_t)bank->n_layers * bank->n_kv_heads * bank->cap);
}
