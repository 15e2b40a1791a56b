// Split-path scorer for decode steps (q_len == 1, at most one victim): one workgroup per (KV head, layer).
// Folds the key-range-split partials of ekv_attn_decode_kernel into the 16-bit output, pulls the exported logits and
// the score rows into LDS by LDS-DMA and runs the same scorer tail as the fused kernel (ekv_decode_tail.h).
// Used when layers are launched one at a time (heads must be split to fill the chip).
#ifdef EKV_TAIL_PROFILE
#define EKV_STAMP(i) do { if (threadIdx.x == 0) stamps[i] = __builtin_readcyclecounter(); } while (0)
#endif
#include "ekv_decode_tail.h"
// EKV_BATCH = 1 (the batch instances): the scorer of a batched decode step — workgroup (head, entry) shadows the per-step
// fields of its arguments from the entry's row of the table (as in ekv_attn_decode.inc) and is the uniform scorer from there on.
// The fold kernel reads no per-step field (partials, split count and output rows are the envelope's): a batch launches the uniform one.
#ifndef EKV_BATCH
#define EKV_BATCH 0
#endif
// EKV_SINK = 1 (the EKV_DECODE_SCORE_SINK lines of the manifest): the scorer behind the split decode kernel's sink instances.  The partials
// it folds carry the virtual key already; the tail, which rebuilds the softmax of the exported logits, takes the sinks (ekv_decode_tail.h).
// The fold kernel is the uniform one (it only folds partials), so these objects export the scorer alone.
#if EKV_SINK && EKV_BATCH
#error "sink scorer instances: one sequence"
#endif
// EKV_HEADS = 1 (the EKV_DECODE_SCORE_HEADS lines of the manifest): the scorer of a decode step over KV heads of different lengths —
// workgroup (head, layer) takes its head's row count from the device table (ekv_kernels.h) and is the uniform scorer from there on.  The
// fold kernel is the uniform one.
#ifndef EKV_HEADS
#define EKV_HEADS 0
#endif
#if EKV_HEADS && (EKV_SINK || EKV_BATCH)
#error "heads scorer instances: no batch table, no sinks"
#endif
#define EKV_HEAD_IDX blockIdx.x
#define ekv_decode_score_kernel EKV_KERNEL_NAME(ekv_decode_score_kernel)
#define ekv_fold_kernel EKV_KERNEL_NAME(ekv_fold_kernel)

namespace {

// (kSNW waves / kSNT threads per scorer workgroup and the LDS plan ekv_decode_score_lds: ekv_geometry.h)
template <int REP, int ITEMS>
__global__ void __launch_bounds__(kSNT) ekv_decode_score_kernel(const EkvScoreArgs EKV_ARG_SC EKV_TB_PARAM EKV_SINK_ONLY(, const float* const sinks) EKV_HEADS_ONLY(, const EkvHeadsArgs heads)) {
  EKV_SHADOW_SC(blockIdx.y)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int h = blockIdx.x, ll = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int T = sc.n_slots, D = sc.head_dim, t_pad = sc.t_pad;
  const bool roco = sc.policy == EKV_POLICY_ROCO;
  const bool scored = roco || sc.policy == EKV_POLICY_H2O_HEAD || sc.policy == EKV_POLICY_TOVA;
  const int off = scored ? sc.score_off : 0;
  const int W = T - off;
  const int w_pad = (int)ekv_align((size_t)W, 256);
  float* s_logit = reinterpret_cast<float*>(smem);
  float* sS = s_logit + (size_t)REP * t_pad;
  float* sQ = sS + w_pad;
  float* sC = sQ + w_pad;
  RedN<kSNW> red;
  red.buf = reinterpret_cast<unsigned long long*>(sS + (size_t)(roco ? 3 : 1) * w_pad);
  red.phase = 0;
  red.lane = lane;
  red.wave = wave;
  const size_t head_row = ((size_t)(sc.layer_begin + ll) * sc.n_kv_heads + h) * sc.cap;
  // REP = the GQA factor rounded up to 1 / 2 / 4 / 8 (ekv_attn_decode.inc); the padding rows repeat the last real head's logits
  const int nrep = (REP == 1 || REP == 2) ? REP : sc.n_q_heads / sc.n_kv_heads;
  const size_t hq0 = (size_t)ll * sc.n_q_heads + (size_t)h * nrep;

#ifdef EKV_TAIL_PROFILE
  unsigned long long* stamps = reinterpret_cast<unsigned long long*>(sc.tova_row) + ((size_t)ll * sc.n_kv_heads + h) * 8;
#endif
  EKV_STAMP(0);
  if (scored) ekv_tail_prefetch_rows<kSNW>(sc, head_row, W, w_pad, roco, sS, sQ, sC);
  if (scored && sc.accumulate) {   // logits rows -> LDS (rows are 256-byte aligned in the workspace)
    const int full = t_pad / 256;
    for (int c = wave; c < full * REP; c += kSNW) {
      const int r = c / full, ch = c % full;
      const float* src = sc.logits + (hq0 + min(r, nrep - 1)) * t_pad + ch * 256 + lane * 4;
      __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(s_logit + (size_t)r * t_pad + ch * 256), 16, 0, 0);
    }
    for (int r = 0; r < REP; ++r)
      for (int j = full * 256 + tid; j < t_pad; j += kSNT) s_logit[(size_t)r * t_pad + j] = sc.logits[(hq0 + min(r, nrep - 1)) * t_pad + j];
  }

  // fold the key-range splits into the attention output
  const int PS = D + 2;
  for (int idx = tid; idx < (sc.skip_fold ? 0 : nrep * D); idx += kSNT) {
    const int r = idx / D, d = idx % D;
    sc.out[(hq0 + r) * D + d] = ekv_to_e(ekv_fold_partials_auto(sc.partials + ((hq0 + r) * sc.n_split) * PS, sc.n_split, PS, d));
  }
  __syncthreads();   // LDS-DMA complete (vmcnt(0) before the barrier) and visible
  EKV_STAMP(1);
  uint32_t* s_hist = reinterpret_cast<uint32_t*>(red.buf + 2 * kSNW * 8);     // roco select scratch: histogram, candidate list
  unsigned long long* s_list = reinterpret_cast<unsigned long long*>(s_hist + 264);
  ekv_decode_tail<REP, ITEMS, kSNW>(sc, ll, h, head_row, T, off, W, s_logit, t_pad, sS, sQ, sC, red, s_hist, s_list, kSNT, nullptr, 0, 0, nrep
                                    EKV_SINK_ONLY(, sinks + (size_t)(sc.layer_begin + ll) * sc.n_q_heads + (size_t)h * nrep));
}

#if !EKV_BATCH && !EKV_SINK && !EKV_HEADS
// Partials of the key-range splits -> 16-bit attention output, nothing else (rows = q_len * n_q_heads per layer).
__global__ void __launch_bounds__(128) ekv_fold_kernel(const EkvScoreArgs sc) {
  const int D = sc.head_dim, PS = D + 2;
  const size_t row = (size_t)blockIdx.y * sc.n_q_heads * sc.q_len + blockIdx.x;
  const float* p0 = sc.partials + row * sc.n_split * PS;
  // (ekv_step.out_*_stride: blockIdx.x = head * q_len + token)
  __half* orow = sc.out + (size_t)blockIdx.y * sc.n_q_heads * sc.q_len * D + (size_t)(blockIdx.x / sc.q_len) * sc.o_hs + (size_t)(blockIdx.x % sc.q_len) * sc.o_ts;
  for (int d = threadIdx.x; d < D; d += 128) orow[d] = ekv_to_e(ekv_fold_partials_auto(p0, sc.n_split, PS, d));
}

#endif

template <int REP, int ITEMS>
hipError_t launch_k(const EkvScoreArgs& sc EKV_TB_DECL EKV_SINK_ONLY(, const float* sinks) EKV_HEADS_ONLY(, const EkvHeadsArgs& heads), int layer_count, hipStream_t s) {
  const size_t lds = ekv_decode_score_lds(REP, sc.t_pad, sc.policy);
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_decode_score_kernel<REP, ITEMS>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((ekv_decode_score_kernel<REP, ITEMS>), dim3(sc.n_kv_heads, layer_count), dim3(kSNT), lds, s, sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_HEADS_ONLY(, heads));
  return hipGetLastError();
}

template <int REP>
hipError_t launch_rep(const EkvScoreArgs& sc EKV_TB_DECL EKV_SINK_ONLY(, const float* sinks) EKV_HEADS_ONLY(, const EkvHeadsArgs& heads), int layer_count, hipStream_t s) {
  // ITEMS = ceil(row width / threads) (a floor here sent T = 2049 to the 6144-wide build: 12 items per thread instead of 5)
  constexpr int I0 = (2304 + kSNT - 1) / kSNT, I1 = (6144 + kSNT - 1) / kSNT;
  return sc.n_slots <= kSNT * I0 ? launch_k<REP, I0>(sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_HEADS_ONLY(, heads), layer_count, s) : launch_k<REP, I1>(sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_HEADS_ONLY(, heads), layer_count, s);
}

#if !EKV_BATCH && !EKV_SINK && !EKV_HEADS
hipError_t launch_fold(const EkvScoreArgs& sc, int layer_count, hipStream_t s) {
  hipLaunchKernelGGL(ekv_fold_kernel, dim3(sc.n_q_heads * sc.q_len, layer_count), dim3(128), 0, s, sc);
  return hipGetLastError();
}
#endif

hipError_t launch_score(const EkvScoreArgs& sc EKV_TB_DECL EKV_SINK_ONLY(, const float* sinks) EKV_HEADS_ONLY(, const EkvHeadsArgs& heads), int layer_count, hipStream_t s) {
  switch (sc.n_q_heads / sc.n_kv_heads) {
    case 1: return launch_rep<1>(sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_HEADS_ONLY(, heads), layer_count, s);
    case 2: return launch_rep<2>(sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_HEADS_ONLY(, heads), layer_count, s);
    case 3: case 4: return launch_rep<4>(sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_HEADS_ONLY(, heads), layer_count, s);
    case 5: case 6: case 7: case 8: return launch_rep<8>(sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_HEADS_ONLY(, heads), layer_count, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

#if EKV_HEADS
hipError_t EKV_FN_ELEM(ekv_launch_decode_score_heads, EKV_ELEM)(const EkvScoreArgs& sc, const EkvHeadsArgs& hd, int count, hipStream_t s) {
  return hd.rows != nullptr ? launch_score(sc, hd, count, s) : hipErrorInvalidValue;
}
#elif EKV_SINK
hipError_t EKV_FN_ELEM(ekv_launch_decode_score_sink, EKV_ELEM)(const EkvScoreArgs& sc, const float* sinks, int count, hipStream_t s) {
  return sinks != nullptr ? launch_score(sc, sinks, count, s) : hipErrorInvalidValue;
}
#else
// tb: the table of a batched step for the batch instances, unused (NULL) otherwise
hipError_t EKV_FN_DECODE_SCORE(ekv_launch_decode_score, EKV_ELEM, EKV_BATCHING)(const EkvScoreArgs& sc, const EkvSeqTable* tb, int count, hipStream_t s) {
  return launch_score(sc EKV_TB_DEREF, count, s);
}
#endif

#if !EKV_BATCH && !EKV_SINK && !EKV_HEADS
hipError_t EKV_FN_ELEM(ekv_launch_fold, EKV_ELEM)(const EkvScoreArgs& sc, int layer_count, hipStream_t s) { return launch_fold(sc, layer_count, s); }
#endif
