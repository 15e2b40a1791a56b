// The step planner (ekv_plan.cpp): every decision about a call of the step family, from the caller's descriptors alone.  Host-only —
// no kernel, no launch, no HIP call — over the families' geometry (ekv_geometry.h); ekv_abi.hip launches what it plans.
#pragma once
#include "ekv_kernels.h"

int check_bank(const ekv_bank* b);
int check_layers(const ekv_bank* b, int begin, int count);

// ---- what a kernel family takes (each rule next to the measurements that set it: ekv_plan.cpp)
bool ekv_attn_decode_supported(int head_dim, int rep);
// Waves per workgroup of the one-launch decode step: 8 for launches of 256 .. 512 heads; 8 as well for more heads when the step runs
// the 8-wave instance with both phase orders (rounds_shape) and the two-round default is on (ekv_plan.cpp); else 4.  EKV_FUSED_NW = 4 | 8
// in the environment overrides.
int ekv_decode_fused_nw(int64_t n_heads_in_launch, bool rounds_shape = false);
// Phase order of the fused decode step's workgroups (ekv_attn_decode.inc, "order K"; the kernel field EkvAttnArgs.fused_order).  Bits
// 0-1: 0 = all F (K+V stream, then the tail), 1 = mixed per CU, 2 = all K (K stream, tail, V stream).  Mixed: bits 4-5 = the number x that
// decides (0 HW_ID.TG_ID, 1 HW_ID.WAVE_ID of wave 0, 2 the workgroup's index in the launch), bits 8-11 a mask m, bits 12-15 a bound b,
// bit 6 = invert: order K when ((x & m) < b) != invert.  Both orders produce the same bits, so a hardware-derived number is as good as any.
// Source 3 (8-wave workgroups): x = the workgroup's index in the launch, which is its place in the dispatch order, and the two nibbles
// are one threshold t in units of 8 workgroups (EKV_ORDER_ROUND_THRESHOLD): order K when (x < t) != invert.  The planner always sets
// invert with this source — order K at or past t — and plans t = 0: every workgroup in order K.  A 4-wave launch never gets source 3:
// an EKV_FUSED_ORDER_RULE that names it is ignored there (the slot rule stays).
int ekv_decode_fused_order(int head_dim, int rep, bool scored, bool slot_rows, int nw, int64_t n_heads_in_launch, int phys_extent);
// Resident rows of a one-launch decode step (the kernel field: bits 16-23 of EkvAttnArgs.fused_order, EKV_RESIDENT_ROWS): the physical
// rows [0, result) of every head are read with default-policy loads, so that they stay in the Infinity Cache from one step to the next;
// the rest are streamed non-temporally.  The largest multiple of 32 rows such that heads * (2 * rows * row_bytes + the score bytes a
// head re-reads every step: `score_rows` float rows, the slot map and the birth row, `cap` words each) fits `budget_bytes`, at most
// phys_extent rounded up to 32; 0 when not even the score bytes fit.  EKV_RESIDENT_ROWS in the environment (an A/B and test knob, read
// once) replaces the byte rule by a row count, capped the same way, under any budget but 0 (0 stays 0).
int ekv_decode_resident_rows(int64_t n_heads_in_launch, int64_t row_bytes, int phys_extent, int cap, int score_rows, int64_t budget_bytes);
// The byte budget of the above: EKV_RESIDENT_MB in the environment (MiB, read once) or the compile-time default, until
// ekv_set_resident_bytes sets one (a negative value returns to the former).
int64_t ekv_resident_budget_bytes();
void ekv_resident_set_budget_bytes(int64_t bytes);
bool ekv_decode_fused_supported(int head_dim, int rep, int n_slots, int t_pad, int l_pad, int n_evict, int cap, int nw);
bool ekv_decode_score_supported(const EkvScoreArgs& sc);
bool ekv_attn_chunk_supported(int head_dim, int rep, int q_len);
bool ekv_chunk_two_pass(int head_dim, int rep, int q_len, int policy, bool scored, bool accumulate, bool rope, int mode);
// the launch runs on the wide-query-block kernel (32x32x16 MFMA, ekv_attn_wide.inc): 33..128 GQA-folded rows per query block,
// plain or RoPE-on-read keys, head_dim 64 / 128, and either the two-pass scheme (rep in {1, 2, 4, 8, 16}) or a step that exports no logits
bool ekv_chunk_wide(int head_dim, int rep, int q_len, bool rope, bool two_pass, bool wants_logits);
// can the scorer of a two-pass wide step run as the tail of its column-sum pass: W score columns, n_wg workgroups per head
bool ekv_wide_tail_supported(int64_t W, int64_t n_wg);
// logits-resident scored chunk step (ekv_attn_resident.inc): the whole step of an unsplit head in ONE launch, K and V read once
bool ekv_attn_resident_supported(int head_dim, int rep, int q_len, int n_slots, int64_t W);
// small-row chunk step with the logits in LDS (ekv_chunk_lds.inc): whole step in one launch, K and V read once
bool ekv_chunk_lds_supported(const ekv_bank* bank, const ekv_step* st, int phys_extent, bool scored);
// kernel launches ekv_launch_attn_chunk issues for these arguments
int ekv_attn_chunk_launches(bool wide, bool rope, bool two_pass, int passes);

// The scalar (shape) fields of the scorer's arguments; call_attend adds the pointers.
EkvScoreArgs score_args(const ekv_bank* bank, const ekv_step* st, const EkvStepPlan& P);
// long_rows: the plan of a long call (ekv_long_*; the rule is stated once, at ekv_plan_step in ekv_plan.cpp)
// capped: the plan of a capped call (ekv_cap_*; the rule is stated once, at resolve_call in ekv_plan.cpp); a sink call (ekv_sink_*) tiles
// its chunk steps by the same rule and passes true as well
// pooled: the plan of a pooled call (ekv_pool_*; the rule is stated once, at resolve_call in ekv_plan.cpp): every in-kernel scorer tail off;
// an adaptive call (ekv_ada_*) plans as the pooled one and passes true as well
int ekv_plan_step(const ekv_bank* bank, const ekv_step* step, EkvStepPlan* P, bool long_rows = false, bool capped = false, bool no_orders = false,
                  bool pooled = false);

// ---- one call path --------------------------------------------------------------------------------------------------------------
// A call of the step family as its entry points spell it, along two independent axes: the row format of the bank (the untyped / _typed
// functions: kv16; ekv_kv8_*: kv8; ekv_kv4_*: kv4; ekv_kv6_*: kv6; ekv_kv84_*: kv84; ekv_kv164_*: kv164 — a quantised call brings the planes of its descriptor) and the batching
// (ekv_*batch_*: the table of a batched decode step).  Which combinations run is the planner's business (resolve_call, over
// kRowsRules) and the manifest's (ekv_instances.def).
struct EkvPlanes {      // what stands for the K/V rows of a quantised bank: the code planes, and the row scales (kv8) / block exponents (kv4, kv6); kv84: K row scales, V block exponents; kv164: the V planes alone (K stays bank->k)
  void *k_codes, *v_codes, *k_aux, *v_aux;
};
inline EkvPlanes ekv_planes(const ekv_kv8* q) { return q ? EkvPlanes{q->k_codes, q->v_codes, q->k_scale, q->v_scale} : EkvPlanes{}; }
inline EkvPlanes ekv_planes(const ekv_kv4* q) { return q ? EkvPlanes{q->k_codes, q->v_codes, q->k_exp, q->v_exp} : EkvPlanes{}; }
inline EkvPlanes ekv_planes(const ekv_kv6* q) { return q ? EkvPlanes{q->k_codes, q->v_codes, q->k_exp, q->v_exp} : EkvPlanes{}; }
inline EkvPlanes ekv_planes(const ekv_kv84* q) { return q ? EkvPlanes{q->k_codes, q->v_codes, q->k_scale, q->v_exp} : EkvPlanes{}; }
inline EkvPlanes ekv_planes(const ekv_kv164* q) { return q ? EkvPlanes{nullptr, q->v_codes, nullptr, q->v_exp} : EkvPlanes{}; }
inline bool ekv_planes_complete(const EkvPlanes& p) { return p.k_codes && p.v_codes && p.k_aux && p.v_aux; }
// ... of a call on `rows`: kv164 has no K planes (its keys are the bank's 16-bit rows, which resolve_call asks for)
inline bool ekv_planes_complete(EkvRows rows, const EkvPlanes& p) { return rows == EKV_ROWS_kv164 ? p.v_codes && p.v_aux : ekv_planes_complete(p); }
struct EkvCall {
  const ekv_bank* bank;
  const ekv_step* step;
  int32_t dtype;
  EkvRows rows;
  EkvPlanes planes;        // rows != kv16: the descriptor's pointers (all NULL for a NULL descriptor; any NULL is an argument error)
  bool batch;              // an ekv_*batch_* call
  const ekv_seq* seqs;
  int32_t n_seq;
  bool long_rows;          // an ekv_long_* call: the long-row scorer where the plan would end in the generic one (16-bit rows, one sequence)
  bool capped;             // an ekv_cap_* call: soft-capped logits (16-bit rows, one sequence, plain keys, head_dim 128 / 256)
  float softcap;           // ... its cap: finite and > 0, or the call is an argument error
  bool sink;               // an ekv_sink_* call: attention sinks (16-bit rows, one sequence, plain keys, head_dim 64 / 128)
  const float* sinks;      // ... the sinks, device fp32 [bank->n_layers][n_q_heads]: only tested for NULL here (an argument error)
  bool window;             // an ekv_win_* call: sliding windows (16-bit rows, one sequence, plain keys; with sinks head_dim 64, alone 128)
  const ekv_win* win;      // ... its struct (include/easykv_hip.h): NULL, NULL tok_pos / windows or a negative window are argument errors
  bool pooled;             // an ekv_pool_* call: pooled selection (16-bit rows, one sequence, h2o_head / tova, no other variant)
  const ekv_pool* pool;    // ... its struct: NULL, radius < 1 or an unknown op are argument errors
  bool adaptive;           // an ekv_ada_* call: adaptive head budgets (16-bit rows, one sequence, h2o_head / tova, no other variant)
  const ekv_ada* ada;      // ... its struct: NULL, NULL n_evict_out, radius < 0, an unknown op or bounds out of order are argument errors
  bool heads;              // an ekv_heads_* call: decode steps over KV heads of different lengths (16-bit rows, plain keys, no other variant)
  const ekv_heads* hd;     // ... its struct: NULL, a NULL pointer, grow < 0 or a host count out of range are argument errors; `rows` is never dereferenced here
};
inline EkvCall step_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype) { return {bank, st, dtype, EKV_ROWS_kv16, {}, false, nullptr, 0}; }
inline EkvCall batch_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_seq* seqs, int32_t n_seq) {
  return {bank, st, dtype, EKV_ROWS_kv16, {}, true, seqs, n_seq};
}
inline EkvCall long_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype) { return {bank, st, dtype, EKV_ROWS_kv16, {}, false, nullptr, 0, true}; }
inline EkvCall cap_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, float softcap) {
  return {bank, st, dtype, EKV_ROWS_kv16, {}, false, nullptr, 0, false, true, softcap};
}
inline EkvCall sink_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const float* sinks) {
  return {bank, st, dtype, EKV_ROWS_kv16, {}, false, nullptr, 0, false, false, 0.f, true, sinks};
}
// (win->s_aux != NULL: the window joins the sink variant; the struct itself is checked in resolve_call)
inline EkvCall win_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_win* win) {
  return {bank, st, dtype, EKV_ROWS_kv16, {}, false, nullptr, 0, false, false, 0.f, win != nullptr && win->s_aux != nullptr, win ? win->s_aux : nullptr, true, win};
}
inline EkvCall pool_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_pool* pool) {
  return {bank, st, dtype, EKV_ROWS_kv16, {}, false, nullptr, 0, false, false, 0.f, false, nullptr, false, nullptr, true, pool};
}
inline EkvCall ada_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_ada* ada) {
  return {bank, st, dtype, EKV_ROWS_kv16, {}, false, nullptr, 0, false, false, 0.f, false, nullptr, false, nullptr, false, nullptr, true, ada};
}
inline EkvCall heads_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_heads* hd) {
  return {bank, st, dtype, EKV_ROWS_kv16, {}, false, nullptr, 0, false, false, 0.f, false, nullptr, false, nullptr, false, nullptr, false, nullptr, true, hd};
}
// the quantised calls: the same two with a row format and its planes
inline EkvCall kv8_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv8* q8) {
  return {bank, st, dtype, EKV_ROWS_kv8, ekv_planes(q8), false, nullptr, 0};
}
inline EkvCall kv4_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv4* q4) {
  return {bank, st, dtype, EKV_ROWS_kv4, ekv_planes(q4), false, nullptr, 0};
}
inline EkvCall kv8_batch_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv8* q8, const ekv_seq* seqs, int32_t n_seq) {
  return {bank, st, dtype, EKV_ROWS_kv8, ekv_planes(q8), true, seqs, n_seq};
}
inline EkvCall kv4_batch_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv4* q4, const ekv_seq* seqs, int32_t n_seq) {
  return {bank, st, dtype, EKV_ROWS_kv4, ekv_planes(q4), true, seqs, n_seq};
}
inline EkvCall kv6_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv6* q6) {
  return {bank, st, dtype, EKV_ROWS_kv6, ekv_planes(q6), false, nullptr, 0};
}
inline EkvCall kv6_batch_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv6* q6, const ekv_seq* seqs, int32_t n_seq) {
  return {bank, st, dtype, EKV_ROWS_kv6, ekv_planes(q6), true, seqs, n_seq};
}
inline EkvCall kv84_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv84* q84) {
  return {bank, st, dtype, EKV_ROWS_kv84, ekv_planes(q84), false, nullptr, 0};
}
inline EkvCall kv84_batch_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv84* q84, const ekv_seq* seqs, int32_t n_seq) {
  return {bank, st, dtype, EKV_ROWS_kv84, ekv_planes(q84), true, seqs, n_seq};
}
inline EkvCall kv164_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv164* q164) {
  return {bank, st, dtype, EKV_ROWS_kv164, ekv_planes(q164), false, nullptr, 0};
}
inline EkvCall kv164_batch_call(const ekv_bank* bank, const ekv_step* st, int32_t dtype, const ekv_kv164* q164, const ekv_seq* seqs, int32_t n_seq) {
  return {bank, st, dtype, EKV_ROWS_kv164, ekv_planes(q164), true, seqs, n_seq};
}
// is `head_dim` one the row format is built for (the table of what each format takes: ekv_plan.cpp, kRowsRules; the conversions ask too)
bool ekv_rows_head_dim(EkvRows rows, int head_dim);

// Everything a call needs, resolved once (resolve_call): check, info, workspace bytes and attend all read it.
struct EkvResolved {
  const ekv_bank* bank;      // the bank planned and launched with; NULL: a quantised call without its planes
  const ekv_step* step;      // the step actually planned: the caller's, or the envelope of a batch or of a heads call
  const EkvSeqTable* tb;     // the table the batch instances receive; NULL for a uniform step
  EkvStepPlan plan;          // rows / batch / fused_order final; zero launches (a batch: zero bytes too) when the call is refused
  ekv_bank bank_q;           // storage of the above, where the call needs its own
  ekv_step env;
  EkvSeqTable table;
};
int resolve_call(const EkvCall& c, EkvResolved* r);
int call_check(const EkvCall& c);
size_t call_workspace_bytes(const EkvCall& c);
// ekv_step_info and its kin: the plan's answers also for a step the call would refuse (launch counts 0 then); argument errors first
// (a long call: entries [10], [11] of EKV_LONG_INFO_N behind the ten of every call)
int call_info(const EkvCall& c, int32_t* info, int32_t n_info);
// ekv_step_resident_rows: the resident rows the call's launch is planned with (0 for every call but a one-launch decode step of the
// instances that have them, and for a step the call would refuse); argument errors as negative codes
int call_resident_rows(const EkvCall& c);
// ekv_step_plan: the split count, and whether the whole step is one launch (0 for a step the call would refuse)
int call_plan(const ekv_bank* bank, const ekv_step* st, int32_t* n_split, int32_t* fused);
