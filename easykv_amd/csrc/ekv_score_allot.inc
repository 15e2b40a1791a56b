// Adaptive head budgets, the allot launch (include/easykv_hip.h, "adaptive head budgets"): between the rank and the select launch of the
// EKV_ADA scorer (ekv_score_select.inc), ONE workgroup per layer turns the layer's eviction total H * n_evict into one count per KV head.
//
// The rank launch left, per (layer, head), the W ranking keys (order-preserving uint32, ekv_fkey) and one class byte per column: 0 forced
// (among the head's evict_min smallest), 1 free, 2 neither (protected, or outside the candidate range).  Every head evicts its forced
// elements; the remaining m = H * (n_evict - evict_min) victims of the layer are the m smallest FREE elements of all heads together in the
// order (key, head, j).  Head h's share is
//     k_h = evict_min + #{free j of h : key < tau} + (its part of the `need` ties at tau, heads in ascending order)
// where tau is the m-th smallest free key and need = m - #{free : key < tau}.  Which j of a head the ties are does not matter here: the
// select launch takes the head's own k_h smallest by (key, j), which are the same elements.
//
// tau: an MSB-first radix select, 8 bits per pass, a 256-bin histogram in LDS per pass (the scheme of blk_kth, ekv_blk_select.h) — over up to
// 64 heads x ~38 400 keys, which stay in L2 / Infinity Cache between the four passes and the counting pass.  Score keys share their leading
// digits, so a wave's 64 keys usually fall into one or two bins: the lanes of a wave are grouped by digit with ballots and ONE lane per
// distinct digit adds the group's size (an ds_add per lane would serialise 64-fold on the one hot bin).  No atomics on global memory; k_h
// goes out by ordinary vector stores.  Runs once per prompt.
//
// Invariant the select rests on: every head has exactly evict_max - evict_min free keys (the rank launch marks exactly evict_max and
// exactly evict_min columns with blk_mark_k_smallest), and the planner admits only n_evict <= evict_max, so the layer holds
// H * (evict_max - evict_min) >= m free keys.  Hence in every pass exactly one lane of wave 0 owns rank kk and rewrites hist[256..258];
// with fewer than m free keys no lane would, and the previous pass's values would be read again.
#include "ekv_common.h"
#include "ekv_kernels.h"

namespace {

constexpr int kNT = EKV_ALLOT_NT;

__global__ void __launch_bounds__(kNT) ekv_score_allot_kernel(const EkvAdaArgs ada, const int H, const int W, const int n_evict) {
  __shared__ uint32_t hist[256 + 4];      // [256] bin, [257] keys below it, [258] keys in it
  __shared__ uint32_t n_lt[64], n_eq[64];      // per head: free keys below tau / equal to tau
  const int ll = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* const keys = ada.keys + (size_t)ll * H * ada.stride;
  const uint8_t* const cls = ada.cls + (size_t)ll * H * ada.stride;
  int32_t* const k_out = ada.k_out + (size_t)ll * H;
  const int m = H * (n_evict - ada.evict_min);
  if (m <= 0) {      // (uniform for the workgroup) nothing to share out: every head evicts its forced elements
    if (tid < H) k_out[tid] = ada.evict_min;
    return;
  }
  const int w_round = (W + kNT - 1) / kNT * kNT;      // every lane takes part in the ballots below

  for (int i = tid; i < 256 + 4; i += kNT) hist[i] = 0;
  if (tid < 64) n_lt[tid] = n_eq[tid] = 0;
  __syncthreads();
  uint32_t prefix = 0;
  int kk = m;      // rank still to find among the free keys that match `prefix`
  for (int shift = 24; shift >= 0; shift -= 8) {
    const uint32_t hi_mask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
    for (int h = 0; h < H; ++h) {
      const uint32_t* const kr = keys + (size_t)h * ada.stride;
      const uint8_t* const cr = cls + (size_t)h * ada.stride;
      for (int j = tid; j < w_round; j += kNT) {
        uint32_t x = 0;
        bool act = j < W && cr[j] == 1;
        if (act) {
          x = kr[j];
          act = (x & hi_mask) == prefix;
        }
        const uint32_t digit = (x >> shift) & 255u;
        unsigned long long todo = __ballot(act);
        while (todo) {      // (wave-uniform) one group of equal digits per turn
          const int leader = __ffsll((long long)todo) - 1;
          const uint32_t d = (uint32_t)__shfl((int)digit, leader, 64);
          const unsigned long long same = __ballot(act && digit == d);
          if (lane == leader) atomicAdd(&hist[d], (uint32_t)__popcll(same));
          todo &= ~same;
        }
      }
    }
    __syncthreads();
    if (wave == 0) {      // lane l owns bins 4l .. 4l + 3; inclusive scan over the lanes; exactly one lane owns rank kk
      const uint32_t c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
      hist[4 * lane] = hist[4 * lane + 1] = hist[4 * lane + 2] = hist[4 * lane + 3] = 0;      // ready for the next pass
      const uint32_t mine = c0 + c1 + c2 + c3;
      uint32_t incl = mine;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
      }
      const uint32_t excl = incl - mine;
      if ((uint32_t)kk > excl && (uint32_t)kk <= incl) {
        uint32_t below = excl, bin = 4 * lane, cnt = c0;
        if ((uint32_t)kk > below + c0) { below += c0; bin++; cnt = c1;
          if ((uint32_t)kk > below + c1) { below += c1; bin++; cnt = c2;
            if ((uint32_t)kk > below + c2) { below += c2; bin++; cnt = c3; } } }
        hist[256] = bin;
        hist[257] = below;
        hist[258] = cnt;
      }
    }
    __syncthreads();
    prefix |= hist[256] << shift;
    kk -= (int)hist[257];
    // (hist[256..258] are rewritten only after the next pass's barrier, by which time every thread has read them)
  }
  const uint32_t tau = prefix;
  const int need = kk;      // of the free keys equal to tau, the first `need` in (head, j) order are victims: 1 <= need <= their number

  // per head: free keys below tau and equal to tau
  for (int h = 0; h < H; ++h) {
    const uint32_t* const kr = keys + (size_t)h * ada.stride;
    const uint8_t* const cr = cls + (size_t)h * ada.stride;
    int lt = 0, eq = 0;
    for (int j = tid; j < w_round; j += kNT) {
      const bool fr = j < W && cr[j] == 1;
      const uint32_t x = fr ? kr[j] : 0xFFFFFFFFu;
      lt += __popcll(__ballot(fr && x < tau));
      eq += __popcll(__ballot(fr && x == tau));
    }
    if (lane == 0) {
      if (lt) atomicAdd(&n_lt[h], (uint32_t)lt);
      if (eq) atomicAdd(&n_eq[h], (uint32_t)eq);
    }
  }
  __syncthreads();
  if (tid < H) {
    int before = 0;
    for (int i = 0; i < tid; ++i) before += (int)n_eq[i];
    const int take = min((int)n_eq[tid], max(0, need - before));
    k_out[tid] = ada.evict_min + (int)n_lt[tid] + take;
  }
}

}  // namespace

hipError_t ekv_launch_score_allot(const EkvScoreArgs& a, const EkvAdaArgs& ada, int layer_count, hipStream_t s) {
  if (a.n_kv_heads > 64 || ada.keys == nullptr || ada.cls == nullptr || ada.k_out == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ekv_score_allot_kernel, dim3(layer_count), dim3(kNT), 0, s, ada, a.n_kv_heads, a.n_slots - a.score_off, a.n_evict);
  return hipGetLastError();
}
