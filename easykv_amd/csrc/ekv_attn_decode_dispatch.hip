// Dispatch over the decode instances of ekv_instances.def: head_dim, keys, element type, row format, batching.
#include "ekv_common.h"
#include "ekv_kernels.h"

// ---- the instances (ekv_instances.def): launcher declarations, then one table entry per line
typedef hipError_t EkvDecodeFn(const EkvAttnArgs&, const EkvSeqTable*, int rep, int count, hipStream_t);
typedef hipError_t EkvFusedFn(const EkvAttnArgs&, const EkvScoreArgs&, const EkvSeqTable*, int rep, int count, int nw, hipStream_t);
typedef hipError_t EkvScoreFn(const EkvScoreArgs&, const EkvSeqTable*, int count, hipStream_t);
typedef hipError_t EkvFoldFn(const EkvScoreArgs&, int layer_count, hipStream_t);
#define EKV_DECODE(d, keys, elem, rows, batching)                            \
  EkvDecodeFn EKV_FN_DECODE(ekv_launch_attn_decode, d, keys, elem, rows, batching); \
  EkvFusedFn EKV_FN_DECODE(ekv_launch_decode_fused, d, keys, elem, rows, batching);
// (the soft-capped decode instances: plain keys, 16-bit rows, one sequence; their launchers carry `cap` where the others name their keys)
#define EKV_DECODE_CAP(elem, d) EKV_DECODE(d, cap, elem, kv16, single)
#define EKV_DECODE_SCORE(elem, batching) EkvScoreFn EKV_FN_DECODE_SCORE(ekv_launch_decode_score, elem, batching);
// (the sink instances: 16-bit rows, plain keys, one sequence; their launchers take the sinks where the others take the table of a batch)
typedef hipError_t EkvSinkDecodeFn(const EkvAttnArgs&, const float* sinks, int rep, int count, hipStream_t);
typedef hipError_t EkvSinkFusedFn(const EkvAttnArgs&, const EkvScoreArgs&, const float* sinks, int rep, int count, int nw, hipStream_t);
typedef hipError_t EkvSinkScoreFn(const EkvScoreArgs&, const float* sinks, int count, hipStream_t);
#define EKV_DECODE_SINK(elem, d)                                   \
  EkvSinkDecodeFn EKV_FN_SINK(ekv_launch_attn_decode, elem, d);    \
  EkvSinkFusedFn EKV_FN_SINK(ekv_launch_decode_fused, elem, d);
#define EKV_DECODE_SCORE_SINK(elem) EkvSinkScoreFn EKV_FN_ELEM(ekv_launch_decode_score_sink, elem);
// (the window instances, alone and with sinks: one signature, `sinks` NULL in the window-alone ones)
typedef hipError_t EkvWinDecodeFn(const EkvAttnArgs&, const float* sinks, const EkvWinArgs&, int rep, int count, hipStream_t);
typedef hipError_t EkvWinFusedFn(const EkvAttnArgs&, const EkvScoreArgs&, const float* sinks, const EkvWinArgs&, int rep, int count, int nw, hipStream_t);
#define EKV_DECODE_WIN(elem, d)                                  \
  EkvWinDecodeFn EKV_FN_WIN(ekv_launch_attn_decode, elem, d);    \
  EkvWinFusedFn EKV_FN_WIN(ekv_launch_decode_fused, elem, d);
#define EKV_DECODE_SINK_WIN(elem, d)                                  \
  EkvWinDecodeFn EKV_FN_SINK_WIN(ekv_launch_attn_decode, elem, d);    \
  EkvWinFusedFn EKV_FN_SINK_WIN(ekv_launch_decode_fused, elem, d);
// (the heads instances: 16-bit rows, plain keys; their launchers take the table's pointer and growth)
typedef hipError_t EkvHeadsDecodeFn(const EkvAttnArgs&, const EkvHeadsArgs&, int rep, int count, hipStream_t);
typedef hipError_t EkvHeadsScoreFn(const EkvScoreArgs&, const EkvHeadsArgs&, int count, hipStream_t);
#define EKV_DECODE_HEADS(elem, d) EkvHeadsDecodeFn EKV_FN_HEADS(ekv_launch_attn_decode, elem, d);
#define EKV_DECODE_SCORE_HEADS(elem) EkvHeadsScoreFn EKV_FN_ELEM(ekv_launch_decode_score_heads, elem);
#include "ekv_instances.def"
EkvFoldFn ekv_launch_fold_f16, ekv_launch_fold_bf16;      // (exported by the `single` scorer instances: the fold reads no per-step field)

namespace {
struct DecodeInstance {
  int head_dim;
  bool rope, capped, bf16;      // (keys: plain | rope | cap)
  EkvRows rows;
  bool batch;
  EkvDecodeFn* attn;
  EkvFusedFn* fused;
};
const DecodeInstance kDecode[] = {
#define EKV_DECODE(d, keys, elem, rows, batching)                                                                   \
  {d, EKV_IS_##keys, EKV_CAPPED_##keys, EKV_IS_##elem, EKV_ROWS_##rows, EKV_IS_##batching, EKV_FN_DECODE(ekv_launch_attn_decode, d, keys, elem, rows, batching), \
   EKV_FN_DECODE(ekv_launch_decode_fused, d, keys, elem, rows, batching)},
#define EKV_DECODE_CAP(elem, d) EKV_DECODE(d, cap, elem, kv16, single)
#include "ekv_instances.def"
};
struct SinkInstance {
  int head_dim;
  bool bf16;
  EkvSinkDecodeFn* attn;
  EkvSinkFusedFn* fused;
};
const SinkInstance kSinkDecode[] = {
#define EKV_DECODE_SINK(elem, d) {d, EKV_IS_##elem, EKV_FN_SINK(ekv_launch_attn_decode, elem, d), EKV_FN_SINK(ekv_launch_decode_fused, elem, d)},
#include "ekv_instances.def"
};
struct SinkScoreInstance {
  bool bf16;
  EkvSinkScoreFn* score;
};
const SinkScoreInstance kSinkScore[] = {
#define EKV_DECODE_SCORE_SINK(elem) {EKV_IS_##elem, EKV_FN_ELEM(ekv_launch_decode_score_sink, elem)},
#include "ekv_instances.def"
};
// A sink launch (ekv_sink_*): 16-bit rows, plain keys, one sequence — its own instances, never another's
const SinkInstance* sink_instance(const EkvAttnArgs& a, const float* sinks, int head_dim, bool bf16) {
  if (sinks == nullptr || a.rope_cos != nullptr) return nullptr;
  for (const SinkInstance& in : kSinkDecode)
    if (in.head_dim == head_dim && in.bf16 == bf16) return &in;
  return nullptr;
}
struct WinInstance {
  int head_dim;
  bool bf16, sink;
  EkvWinDecodeFn* attn;
  EkvWinFusedFn* fused;
};
const WinInstance kWinDecode[] = {
#define EKV_DECODE_WIN(elem, d) {d, EKV_IS_##elem, false, EKV_FN_WIN(ekv_launch_attn_decode, elem, d), EKV_FN_WIN(ekv_launch_decode_fused, elem, d)},
#define EKV_DECODE_SINK_WIN(elem, d) \
  {d, EKV_IS_##elem, true, EKV_FN_SINK_WIN(ekv_launch_attn_decode, elem, d), EKV_FN_SINK_WIN(ekv_launch_decode_fused, elem, d)},
#include "ekv_instances.def"
};
// A window launch (ekv_win_*): its own instances, with or without sinks, never another's
const WinInstance* win_instance(const EkvAttnArgs& a, const float* sinks, const EkvWinArgs& win, int head_dim, bool bf16) {
  if (win.tok_pos == nullptr || win.windows == nullptr || a.rope_cos != nullptr) return nullptr;
  for (const WinInstance& in : kWinDecode)
    if (in.head_dim == head_dim && in.bf16 == bf16 && in.sink == (sinks != nullptr)) return &in;
  return nullptr;
}
struct HeadsInstance {
  int head_dim;
  bool bf16;
  EkvHeadsDecodeFn* attn;
};
const HeadsInstance kHeadsDecode[] = {
#define EKV_DECODE_HEADS(elem, d) {d, EKV_IS_##elem, EKV_FN_HEADS(ekv_launch_attn_decode, elem, d)},
#include "ekv_instances.def"
};
struct HeadsScoreInstance {
  bool bf16;
  EkvHeadsScoreFn* score;
};
const HeadsScoreInstance kHeadsScore[] = {
#define EKV_DECODE_SCORE_HEADS(elem) {EKV_IS_##elem, EKV_FN_ELEM(ekv_launch_decode_score_heads, elem)},
#include "ekv_instances.def"
};
struct ScoreInstance {
  bool bf16, batch;
  EkvScoreFn* score;
};
const ScoreInstance kDecodeScore[] = {
#define EKV_DECODE_SCORE(elem, batching) {EKV_IS_##elem, EKV_IS_##batching, EKV_FN_DECODE_SCORE(ekv_launch_decode_score, elem, batching)},
#include "ekv_instances.def"
};

// The instance of a decode launch, or nullptr (hipErrorInvalidValue) for a combination the manifest does not hold or the arguments do
// not fit: quantised rows need plain keys and their auxiliary planes (kv8: the row scales; kv4 / kv6: the block exponents, and a GQA factor of
// at most 4; kv84: the K row scales and the V block exponents; kv164: the V block exponents), bf16 and batches have no RoPE-on-read build, a batch runs on the ordered layout (the planner refuses all of these before
// a launch).  The row format and the batching are independent fields: a batched step on quantised rows looks up its own instance,
// which takes the table and the planes together, and a combination without a line of the manifest finds nothing.
// A capped launch (ekv_cap_*): 16-bit rows, plain keys, one sequence, a cap that is finite and > 0 — its own instances, never another's.
const DecodeInstance* decode_instance(const EkvAttnArgs& a, const EkvSeqTable* tb, int head_dim, bool bf16, EkvRows rows, bool fused_slot_rows,
                                      bool capped) {
  const bool rope = a.rope_cos != nullptr, batch = tb != nullptr;
  if (capped && (rope || batch || rows != EKV_ROWS_kv16 || !(a.softcap > 0.f) || a.softcap > 3.0e38f)) return nullptr;
  if (rows == EKV_ROWS_kv8 && (rope || a.k_scale == nullptr || a.v_scale == nullptr)) return nullptr;
  if ((rows == EKV_ROWS_kv4 || rows == EKV_ROWS_kv6) && (rope || a.k_exp == nullptr || a.v_exp == nullptr || a.n_q_heads > 4 * a.n_kv_heads)) return nullptr;
  if (rows == EKV_ROWS_kv84 && (rope || a.k_scale == nullptr || a.v_exp == nullptr)) return nullptr;
  if (rows == EKV_ROWS_kv164 && (rope || a.v_exp == nullptr)) return nullptr;
  if (bf16 && rope) return nullptr;
  if (batch && (rope || fused_slot_rows)) return nullptr;
  for (const DecodeInstance& in : kDecode)
    if (in.head_dim == head_dim && in.rope == rope && in.capped == capped && in.bf16 == bf16 && in.rows == rows && in.batch == batch) return &in;
  return nullptr;
}
}  // namespace

hipError_t ekv_launch_attn_decode(const EkvAttnArgs& a, const EkvSeqTable* tb, int head_dim, int count, hipStream_t s, bool bf16, EkvRows rows,
                                  bool capped) {
  const DecodeInstance* in = decode_instance(a, tb, head_dim, bf16, rows, false, capped);
  return in ? in->attn(a, tb, a.n_q_heads / a.n_kv_heads, count, s) : hipErrorInvalidValue;
}

// The whole decode step in one launch (which steps, how many waves, which phase order: ekv_plan.cpp)
hipError_t ekv_launch_decode_fused(const EkvAttnArgs& a, const EkvScoreArgs& sc, const EkvSeqTable* tb, int head_dim, int count, int nw,
                                   hipStream_t s, bool bf16, EkvRows rows, bool capped) {
  const DecodeInstance* in = decode_instance(a, tb, head_dim, bf16, rows, sc.birth != nullptr, capped);
  return in ? in->fused(a, sc, tb, a.n_q_heads / a.n_kv_heads, count, nw, s) : hipErrorInvalidValue;
}

// ---- scorer and fold of the split path (ekv_decode_score.inc)
hipError_t ekv_launch_decode_score(const EkvScoreArgs& sc, const EkvSeqTable* tb, int count, hipStream_t s, bool bf16) {
  for (const ScoreInstance& in : kDecodeScore)
    if (in.bf16 == bf16 && in.batch == (tb != nullptr)) return in.score(sc, tb, count, s);
  return hipErrorInvalidValue;
}

hipError_t ekv_launch_fold(const EkvScoreArgs& sc, int layer_count, hipStream_t s, bool bf16) {
  return (bf16 ? ekv_launch_fold_bf16 : ekv_launch_fold_f16)(sc, layer_count, s);
}

// ---- attention sinks (the ekv_sink_* calls): the split kernel, the one-launch kernel and the split path's scorer
hipError_t ekv_launch_attn_decode_sink(const EkvAttnArgs& a, const float* sinks, int head_dim, int count, hipStream_t s, bool bf16) {
  const SinkInstance* in = sink_instance(a, sinks, head_dim, bf16);
  return in ? in->attn(a, sinks, a.n_q_heads / a.n_kv_heads, count, s) : hipErrorInvalidValue;
}

hipError_t ekv_launch_decode_fused_sink(const EkvAttnArgs& a, const EkvScoreArgs& sc, const float* sinks, int head_dim, int count, int nw,
                                        hipStream_t s, bool bf16) {
  const SinkInstance* in = sink_instance(a, sinks, head_dim, bf16);
  return in ? in->fused(a, sc, sinks, a.n_q_heads / a.n_kv_heads, count, nw, s) : hipErrorInvalidValue;
}

hipError_t ekv_launch_decode_score_sink(const EkvScoreArgs& sc, const float* sinks, int count, hipStream_t s, bool bf16) {
  for (const SinkScoreInstance& in : kSinkScore)
    if (in.bf16 == bf16) return in.score(sc, sinks, count, s);
  return hipErrorInvalidValue;
}

// ---- KV heads of different lengths (the ekv_heads_* calls): the split kernel and the split path's scorer — their own instances, never another's
hipError_t ekv_launch_attn_decode_heads(const EkvAttnArgs& a, const EkvHeadsArgs& hd, int head_dim, int count, hipStream_t s, bool bf16) {
  if (a.rope_cos != nullptr) return hipErrorInvalidValue;
  for (const HeadsInstance& in : kHeadsDecode)
    if (in.head_dim == head_dim && in.bf16 == bf16) return in.attn(a, hd, a.n_q_heads / a.n_kv_heads, count, s);
  return hipErrorInvalidValue;
}

hipError_t ekv_launch_decode_score_heads(const EkvScoreArgs& sc, const EkvHeadsArgs& hd, int count, hipStream_t s, bool bf16) {
  for (const HeadsScoreInstance& in : kHeadsScore)
    if (in.bf16 == bf16) return in.score(sc, hd, count, s);
  return hipErrorInvalidValue;
}

// ---- sliding windows (the ekv_win_* calls): the split kernel and the one-launch kernel (the scorer behind the split kernel is the plain
// or the sink one: ekv_kernels.h)
hipError_t ekv_launch_attn_decode_win(const EkvAttnArgs& a, const float* sinks, const EkvWinArgs& win, int head_dim, int count, hipStream_t s, bool bf16) {
  const WinInstance* in = win_instance(a, sinks, win, head_dim, bf16);
  return in ? in->attn(a, sinks, win, a.n_q_heads / a.n_kv_heads, count, s) : hipErrorInvalidValue;
}

hipError_t ekv_launch_decode_fused_win(const EkvAttnArgs& a, const EkvScoreArgs& sc, const float* sinks, const EkvWinArgs& win, int head_dim, int count,
                                       int nw, hipStream_t s, bool bf16) {
  const WinInstance* in = win_instance(a, sinks, win, head_dim, bf16);
  return in ? in->fused(a, sc, sinks, win, a.n_q_heads / a.n_kv_heads, count, nw, s) : hipErrorInvalidValue;
}
