// Dispatch over the decode instances of ekv_instances.def: head_dim, keys, element type, row format, batching.
#include <cstdio>
#include <cstdlib>

#include "ekv_common.h"
#include "ekv_kernels.h"
#include "ekv_decode_stream.h"      // (EkvDecodeGeom: the LDS plan of the one-launch kernel)

// Mixed phase orders of the fused decode step: the default mode and rule (ekv_decode_fused_order).  Rule: order K for the workgroups
// whose hardware slot on the CU (HW_ID.TG_ID) has bit 1 set — slots 2 and 3 of the four a CU holds.  The four workgroups of a CU do
// not advance together: the oldest slot is served first and ends its stream ~85 us before the youngest (cycle stamps,
// docs/TUNING.md §8 "phase orders"), so the tails of slots 0 and 1 already run under their neighbours' streams; what is exposed is
// the tail of the LAST workgroup.  With slots 2 and 3 in order K the last thing a CU does is stream V.  Measured (us per launch,
// Llama2-7B shape): all F 185.6, slots {2, 3} 175.1, {1, 2, 3} 176.4, {3} 178.0, {1, 3} 180.3, all K 181.4, {0, 2} 189.7, {0, 1} 191.4.
#ifndef EKV_FUSED_ORDER_DEFAULT
#define EKV_FUSED_ORDER_DEFAULT 1
#endif
#define EKV_FUSED_ORDER_SRC 0
#define EKV_FUSED_ORDER_MASK 2
#define EKV_FUSED_ORDER_BOUND 2
#define EKV_FUSED_ORDER_INVERT 1

// ---- the instances (ekv_instances.def): launcher declarations, then one table entry per line
typedef hipError_t EkvDecodeFn(const EkvAttnArgs&, const EkvSeqTable*, int rep, int count, hipStream_t);
typedef hipError_t EkvFusedFn(const EkvAttnArgs&, const EkvScoreArgs&, const EkvSeqTable*, int rep, int count, int nw, hipStream_t);
typedef hipError_t EkvScoreFn(const EkvScoreArgs&, const EkvSeqTable*, int count, hipStream_t);
typedef hipError_t EkvFoldFn(const EkvScoreArgs&, int layer_count, hipStream_t);
#define EKV_DECODE(d, keys, elem, rows, batching)                            \
  EkvDecodeFn EKV_FN_DECODE(ekv_launch_attn_decode, d, keys, elem, rows, batching); \
  EkvFusedFn EKV_FN_DECODE(ekv_launch_decode_fused, d, keys, elem, rows, batching);
#define EKV_DECODE_SCORE(elem, batching) EkvScoreFn EKV_FN_DECODE_SCORE(ekv_launch_decode_score, elem, batching);
#include "ekv_instances.def"
EkvFoldFn ekv_launch_fold_f16, ekv_launch_fold_bf16;      // (exported by the `single` scorer instances: the fold reads no per-step field)

namespace {
struct DecodeInstance {
  int head_dim;
  bool rope, bf16, kv8, batch;
  EkvDecodeFn* attn;
  EkvFusedFn* fused;
};
const DecodeInstance kDecode[] = {
#define EKV_DECODE(d, keys, elem, rows, batching)                                                                   \
  {d, EKV_IS_##keys, EKV_IS_##elem, EKV_IS_##rows, EKV_IS_##batching, EKV_FN_DECODE(ekv_launch_attn_decode, d, keys, elem, rows, batching), \
   EKV_FN_DECODE(ekv_launch_decode_fused, d, keys, elem, rows, batching)},
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
// not fit: kv8 needs plain keys and the scale planes, bf16 and batches have no RoPE-on-read build, a batch runs on the ordered layout
// (the planner refuses all of these before a launch).
const DecodeInstance* decode_instance(const EkvAttnArgs& a, const EkvSeqTable* tb, int head_dim, bool bf16, bool kv8, bool fused_slot_rows) {
  const bool rope = a.rope_cos != nullptr, batch = tb != nullptr;
  if (kv8 && (rope || a.k_scale == nullptr || a.v_scale == nullptr)) return nullptr;
  if (bf16 && rope) return nullptr;
  if (batch && (rope || fused_slot_rows)) return nullptr;
  for (const DecodeInstance& in : kDecode)
    if (in.head_dim == head_dim && in.rope == rope && in.bf16 == bf16 && in.kv8 == kv8 && in.batch == batch) return &in;
  return nullptr;
}
}  // namespace

// any GQA factor (repeat_kv, llama_patch.py:19-29): factors <= 8 on the build of the next power of two, wider ones in groups of 8
bool ekv_attn_decode_supported(int head_dim, int rep) {
  return (head_dim == 32 || head_dim == 64 || head_dim == 96 || head_dim == 128) && rep >= 1;
}

hipError_t ekv_launch_attn_decode(const EkvAttnArgs& a, const EkvSeqTable* tb, int head_dim, int count, hipStream_t s, bool bf16, bool kv8) {
  const DecodeInstance* in = decode_instance(a, tb, head_dim, bf16, kv8, false);
  return in ? in->attn(a, tb, a.n_q_heads / a.n_kv_heads, count, s) : hipErrorInvalidValue;
}

// The whole decode step in one launch: possible when a head is not split, at most one victim, and the row fits.
// nw = 4: up to four workgroups per CU (LDS <= 80 KB keeps >= 2); nw = 8: one or two workgroups per CU.
int ekv_decode_fused_nw(int n_heads_in_launch) {
  static const int force = [] { const char* e = std::getenv("EKV_FUSED_NW"); return e ? std::atoi(e) : 0; }();   // (A/B knob)
  if (force == 4 || force == 8) return force;
  return (n_heads_in_launch >= 256 && n_heads_in_launch <= 512) ? 8 : 4;
}

// Which phase order the workgroups of a one-launch decode step run in (ekv_kernels.h).  Order K exists in the instance that serves the
// flagship shape: head_dim 128, one query head per KV head, 4-wave workgroups, slot-indexed rows of at most 2304 physical rows, and only
// a scored policy has a tail to move.  Mixed needs at least two workgroups on a CU (256 CUs): per-layer and short stage launches keep
// order F.  EKV_FUSED_ORDER = 0 all F / 1 mixed / 2 all K and EKV_FUSED_ORDER_RULE = source, mask, bound, invert as "s,m,b,i" (A/B knobs, read once).
int ekv_decode_fused_order(int head_dim, int rep, bool scored, bool slot_rows, int nw, int n_heads_in_launch, int phys_extent) {
  static const int knob = [] { const char* e = std::getenv("EKV_FUSED_ORDER"); return e ? std::atoi(e) : EKV_FUSED_ORDER_DEFAULT; }();
  static const int rule = [] {
    int s = EKV_FUSED_ORDER_SRC, m = EKV_FUSED_ORDER_MASK, b = EKV_FUSED_ORDER_BOUND, inv = EKV_FUSED_ORDER_INVERT;
    if (const char* e = std::getenv("EKV_FUSED_ORDER_RULE")) std::sscanf(e, "%d,%d,%d,%d", &s, &m, &b, &inv);
    return ((s & 3) << 4) | ((inv & 1) << 6) | ((m & 15) << 8) | ((b & 15) << 12);
  }();
  if (knob <= 0 || knob > 2 || head_dim != 128 || rep != 1 || !scored || !slot_rows || nw != 4 || phys_extent > 2304) return 0;
  if (knob == 2) return 2;
  return n_heads_in_launch >= 512 ? (1 | rule) : 0;
}

bool ekv_decode_fused_supported(int head_dim, int rep, int n_slots, int t_pad, int l_pad, int n_evict, int cap, int nw) {
  // (the slot map and the score rows are fetched 16 bytes at a time: rows must be 16-byte aligned)
  if (!ekv_attn_decode_supported(head_dim, rep) || rep > 8 || n_evict > 1 || n_slots > 256 * 24 || (cap & 3) != 0 || cap < 16) return false;
  size_t lds = 1 << 30;
  switch (head_dim) {
    case 32: lds = ekv_fused_lds_max<32>(rep, t_pad, l_pad, nw); break;
    case 64: lds = ekv_fused_lds_max<64>(rep, t_pad, l_pad, nw); break;
    case 96: lds = ekv_fused_lds_max<96>(rep, t_pad, l_pad, nw); break;
    case 128: lds = ekv_fused_lds_max<128>(rep, t_pad, l_pad, nw); break;
  }
  return lds <= (nw == 8 ? 150 : 80) * 1024;   // 80 KB still leaves two 4-wave workgroups per CU
}

hipError_t ekv_launch_decode_fused(const EkvAttnArgs& a, const EkvScoreArgs& sc, const EkvSeqTable* tb, int head_dim, int count, int nw,
                                   hipStream_t s, bool bf16, bool kv8) {
  const DecodeInstance* in = decode_instance(a, tb, head_dim, bf16, kv8, sc.birth != nullptr);
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
