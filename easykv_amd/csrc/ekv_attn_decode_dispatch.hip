// head_dim / rope dispatch over the per-(D, rope) decode objects.
#include <cstdio>
#include <cstdlib>

#include "ekv_common.h"
#include "ekv_kernels.h"

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

hipError_t ekv_launch_attn_decode_d32_plain(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d32_plain(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
size_t ekv_fused_lds_d32_plain(int, int, int, int);
hipError_t ekv_launch_attn_decode_d32_rope(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d32_rope(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
size_t ekv_fused_lds_d32_rope(int, int, int, int);
hipError_t ekv_launch_attn_decode_d64_plain(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d64_plain(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
size_t ekv_fused_lds_d64_plain(int, int, int, int);
hipError_t ekv_launch_attn_decode_d64_rope(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d64_rope(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
size_t ekv_fused_lds_d64_rope(int, int, int, int);
hipError_t ekv_launch_attn_decode_d96_plain(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d96_plain(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
size_t ekv_fused_lds_d96_plain(int, int, int, int);
hipError_t ekv_launch_attn_decode_d96_rope(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d96_rope(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
size_t ekv_fused_lds_d96_rope(int, int, int, int);
hipError_t ekv_launch_attn_decode_d128_plain(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d128_plain(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
size_t ekv_fused_lds_d128_plain(int, int, int, int);
hipError_t ekv_launch_attn_decode_d128_rope(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d128_rope(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
size_t ekv_fused_lds_d128_rope(int, int, int, int);
hipError_t ekv_launch_attn_decode_d32_plain_bf16(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d32_plain_bf16(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
hipError_t ekv_launch_attn_decode_d64_plain_bf16(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d64_plain_bf16(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
hipError_t ekv_launch_attn_decode_d96_plain_bf16(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d96_plain_bf16(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
hipError_t ekv_launch_attn_decode_d128_plain_bf16(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d128_plain_bf16(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
// FP8-row ("kv8") instances: plain keys, head_dim 64 / 128, fp16 or bf16 queries / outputs
hipError_t ekv_launch_attn_decode_d64_plain_kv8(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d64_plain_kv8(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
hipError_t ekv_launch_attn_decode_d128_plain_kv8(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d128_plain_kv8(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
hipError_t ekv_launch_attn_decode_d64_plain_bf16_kv8(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d64_plain_bf16_kv8(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
hipError_t ekv_launch_attn_decode_d128_plain_bf16_kv8(const EkvAttnArgs&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d128_plain_bf16_kv8(const EkvAttnArgs&, const EkvScoreArgs&, int, int, int, hipStream_t);
// batch instances (batched decode steps, ekv_seq): plain keys, every head_dim, fp16 or bf16
hipError_t ekv_launch_attn_decode_d32_plain_batch(const EkvAttnArgs&, const EkvSeqTable&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d32_plain_batch(const EkvAttnArgs&, const EkvScoreArgs&, const EkvSeqTable&, int, int, int, hipStream_t);
hipError_t ekv_launch_attn_decode_d32_plain_bf16_batch(const EkvAttnArgs&, const EkvSeqTable&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d32_plain_bf16_batch(const EkvAttnArgs&, const EkvScoreArgs&, const EkvSeqTable&, int, int, int, hipStream_t);
hipError_t ekv_launch_attn_decode_d64_plain_batch(const EkvAttnArgs&, const EkvSeqTable&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d64_plain_batch(const EkvAttnArgs&, const EkvScoreArgs&, const EkvSeqTable&, int, int, int, hipStream_t);
hipError_t ekv_launch_attn_decode_d64_plain_bf16_batch(const EkvAttnArgs&, const EkvSeqTable&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d64_plain_bf16_batch(const EkvAttnArgs&, const EkvScoreArgs&, const EkvSeqTable&, int, int, int, hipStream_t);
hipError_t ekv_launch_attn_decode_d96_plain_batch(const EkvAttnArgs&, const EkvSeqTable&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d96_plain_batch(const EkvAttnArgs&, const EkvScoreArgs&, const EkvSeqTable&, int, int, int, hipStream_t);
hipError_t ekv_launch_attn_decode_d96_plain_bf16_batch(const EkvAttnArgs&, const EkvSeqTable&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d96_plain_bf16_batch(const EkvAttnArgs&, const EkvScoreArgs&, const EkvSeqTable&, int, int, int, hipStream_t);
hipError_t ekv_launch_attn_decode_d128_plain_batch(const EkvAttnArgs&, const EkvSeqTable&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d128_plain_batch(const EkvAttnArgs&, const EkvScoreArgs&, const EkvSeqTable&, int, int, int, hipStream_t);
hipError_t ekv_launch_attn_decode_d128_plain_bf16_batch(const EkvAttnArgs&, const EkvSeqTable&, int, int, hipStream_t);
hipError_t ekv_launch_decode_fused_d128_plain_bf16_batch(const EkvAttnArgs&, const EkvScoreArgs&, const EkvSeqTable&, int, int, int, hipStream_t);

// any GQA factor (repeat_kv, llama_patch.py:19-29): factors <= 8 on the build of the next power of two, wider ones in groups of 8
bool ekv_attn_decode_supported(int head_dim, int rep) {
  return (head_dim == 32 || head_dim == 64 || head_dim == 96 || head_dim == 128) && rep >= 1;
}

// (bf16: plain keys only — the planner refuses RoPE-on-read steps of a bf16 bank)
#define EKV_DISPATCH(fn, ...)                                                                                      \
  switch (head_dim) {                                                                                              \
    case 32: return bf16 ? fn##32_plain_bf16(__VA_ARGS__) : rope ? fn##32_rope(__VA_ARGS__) : fn##32_plain(__VA_ARGS__);    \
    case 64: return bf16 ? fn##64_plain_bf16(__VA_ARGS__) : rope ? fn##64_rope(__VA_ARGS__) : fn##64_plain(__VA_ARGS__);    \
    case 96: return bf16 ? fn##96_plain_bf16(__VA_ARGS__) : rope ? fn##96_rope(__VA_ARGS__) : fn##96_plain(__VA_ARGS__);    \
    case 128: return bf16 ? fn##128_plain_bf16(__VA_ARGS__) : rope ? fn##128_rope(__VA_ARGS__) : fn##128_plain(__VA_ARGS__); \
  }

// (kv8: plain keys, head_dim 64 / 128, rows + scales — the planner refuses everything else before a launch)
#define EKV_DISPATCH_KV8(fn, ...)                                                                        \
  if (kv8) {                                                                                             \
    if (rope || a.k_scale == nullptr || a.v_scale == nullptr) return hipErrorInvalidValue;               \
    switch (head_dim) {                                                                                  \
      case 64: return bf16 ? fn##64_plain_bf16_kv8(__VA_ARGS__) : fn##64_plain_kv8(__VA_ARGS__);         \
      case 128: return bf16 ? fn##128_plain_bf16_kv8(__VA_ARGS__) : fn##128_plain_kv8(__VA_ARGS__);      \
    }                                                                                                    \
    return hipErrorInvalidValue;                                                                         \
  }

hipError_t ekv_launch_attn_decode(const EkvAttnArgs& a, int head_dim, int layer_count, hipStream_t s, bool bf16, bool kv8) {
  const int rep = a.n_q_heads / a.n_kv_heads;
  const bool rope = a.rope_cos != nullptr;
  EKV_DISPATCH_KV8(ekv_launch_attn_decode_d, a, rep, layer_count, s)
  if (bf16 && rope) return hipErrorInvalidValue;
  EKV_DISPATCH(ekv_launch_attn_decode_d, a, rep, layer_count, s)
  return hipErrorInvalidValue;
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
    case 32: lds = ekv_fused_lds_d32_plain(rep, t_pad, l_pad, nw); break;
    case 64: lds = ekv_fused_lds_d64_plain(rep, t_pad, l_pad, nw); break;
    case 96: lds = ekv_fused_lds_d96_plain(rep, t_pad, l_pad, nw); break;
    case 128: lds = ekv_fused_lds_d128_plain(rep, t_pad, l_pad, nw); break;
  }
  return lds <= (nw == 8 ? 150 : 80) * 1024;   // 80 KB still leaves two 4-wave workgroups per CU
}

hipError_t ekv_launch_decode_fused(const EkvAttnArgs& a, const EkvScoreArgs& sc, int head_dim, int layer_count, int nw,
                                   hipStream_t s, bool bf16, bool kv8) {
  const int rep = a.n_q_heads / a.n_kv_heads;
  const bool rope = a.rope_cos != nullptr;
  EKV_DISPATCH_KV8(ekv_launch_decode_fused_d, a, sc, rep, layer_count, nw, s)
  if (bf16 && rope) return hipErrorInvalidValue;
  EKV_DISPATCH(ekv_launch_decode_fused_d, a, sc, rep, layer_count, nw, s)
  return hipErrorInvalidValue;
}

// batched decode steps: the batch instances of the two kernels above (plain keys; the planner refuses everything else)
#define EKV_DISPATCH_BATCH(fn, ...)                                                                      \
  switch (head_dim) {                                                                                    \
    case 32: return bf16 ? fn##32_plain_bf16_batch(__VA_ARGS__) : fn##32_plain_batch(__VA_ARGS__);       \
    case 64: return bf16 ? fn##64_plain_bf16_batch(__VA_ARGS__) : fn##64_plain_batch(__VA_ARGS__);       \
    case 96: return bf16 ? fn##96_plain_bf16_batch(__VA_ARGS__) : fn##96_plain_batch(__VA_ARGS__);       \
    case 128: return bf16 ? fn##128_plain_bf16_batch(__VA_ARGS__) : fn##128_plain_batch(__VA_ARGS__);    \
  }

hipError_t ekv_launch_attn_decode_batch(const EkvAttnArgs& a, const EkvSeqTable& tb, int head_dim, int n_seq, hipStream_t s, bool bf16) {
  const int rep = a.n_q_heads / a.n_kv_heads;
  if (a.rope_cos != nullptr) return hipErrorInvalidValue;
  EKV_DISPATCH_BATCH(ekv_launch_attn_decode_d, a, tb, rep, n_seq, s)
  return hipErrorInvalidValue;
}

hipError_t ekv_launch_decode_fused_batch(const EkvAttnArgs& a, const EkvScoreArgs& sc, const EkvSeqTable& tb, int head_dim, int n_seq, int nw,
                                         hipStream_t s, bool bf16) {
  const int rep = a.n_q_heads / a.n_kv_heads;
  if (a.rope_cos != nullptr || sc.birth != nullptr) return hipErrorInvalidValue;
  EKV_DISPATCH_BATCH(ekv_launch_decode_fused_d, a, sc, tb, rep, n_seq, nw, s)
  return hipErrorInvalidValue;
}
