// K2r: a scored chunk step whose LOGITS stay in the register file — one launch, one workgroup per (KV head, layer), K and V read ONCE.
//
// Same contract as a two-pass step of ekv_attn_wide.inc (easykv/llama_patch.py:198-222, mistral_patch.py:144-169 for q_len = stride;
// the K/V append of DynamicCache.update, llama_patch.py:193-196; column sums of the GQA-folded probabilities easykv/easykv.py:443-457,
// :173-186; accumulate / select / compact :443-499 through ekv_wide_tail.h) for the steps that are small enough: 9..64 GQA-folded
// query rows against T <= 1280 keys, or up to 32 rows against T <= 2560 (the LONG shape below) — BASELINE configs[2] (Mistral GQA x 4,
// stride 16, budget 0.3 of 4096: 64 rows x 1248 keys, 256 (head, layer) pairs = ONE workgroup per CU).
//
// Why: at that shape the two-pass scheme is three serial chains on every CU — the K + V pass (41 us, one 32 KB tile pair in flight per
// CU), the K-only column-sum pass (20 us) and the scorer tail (19 us on 256 threads) — and nothing runs beside them.  A CU's register
// file is 512 KB: 64 x 1280 fp32 logits are 320 KB, i.e. 160 accumulator registers per lane of a 512-thread workgroup.  So:
//   1. K pass   K tiles (128 keys, 32 KB) stream through a 3-deep LDS ring by LDS-DMA; wave (wq, wk) keeps S = Q.K^T of its 32 rows x
//               32 keys of EVERY tile in registers (s[tile], "query = register, key = lane": column sums are lane-local).
//   2. maxima   exact row maxima over the resident logits (DPP + one LDS exchange over the four key waves).  No running maximum, no
//               rescaling, nothing is re-computed.
//   3. V pass   V tiles through the same ring (the first ones are in flight since the end of the K pass).  Per tile: p' = 2^((s - m)c)
//               of the tile in place (16 exponentials per lane, under the wait for the stream), p' as an fp16 P^T tile to LDS, and
//               EVERY wave accumulates one 32 (d) x 32 (q) block of O^T = V^T.P^T over all keys — no cross-wave reduction of O.
//   4. sums     L = sum p' per row (DPP + LDS), then the column sums of pbar = mean over the GQA group of p' / L and of pbar^2 (the
//               arithmetic of ekv_attn_wide.inc's column-sum pass, same order of the sums) -> LDS, complete for the head: no partial
//               rows, no global round trip.  The chunk's own rows for the append and the scorer's score rows are requested in front
//               of this phase and consumed behind it.
//   5. output   O / L, fp16; the chunk's own K / V rows -> their cache slots.
//   6. scorer   ekv_wide_tail.h on 512 threads, column sums read from LDS.
// HBM traffic = K + V once (the algorithmic minimum: no K re-read), two tiles in flight per CU at all times, and
// ekv_step_info.n_launches = 1.
// Query blocks of 9..32 rows run on the same instance (the second query wave of a key-wave pair then holds no rows: the step is
// bound by its stream, not by the MFMAs): measured against the 16x16 kernel + scorer tail they replace (us per 32-layer step, T ~
// 1240): Mistral shape, stride 8 / 4 (32 / 16 rows) 44.0 / 43.3 against 71.5-73.9 / 61.5-62.2; Llama2-7B shape (1024 heads), stride 32
// / 16: 175.8-184.2 / 171.1-177.5 against 212.5-213.6 / 175.2-176.4; 8 KV heads x 4 layers, stride 8: 37.7 against 44.9.
// The LONG shape (<= 32 rows, 1280 < T <= 2560: budget 0.5 of a 4 k prompt at strides 8 .. 32) against the same paths, T ~ 2064-2112:
// Mistral shape, stride 8: 63.7-64.0 against 110.7-111.8 us; Llama2-7B shape, stride 32 / 16: 272.8-286.6 / 272.0 against 371.3-371.9 /
// 311.4-316.1 us.
// Measured (MI355X, configs[2] shape, 32 layers x 8 KV heads per launch): 47.6-47.9 us per step against 81.9-82.4 us for the two-pass
// step (one pass 41 + column-sum pass 20 + tail 19); cycle stamps per head (-DEKR_PROFILE, tools/experiments/exp_resident_prof.py):
// prologue 6.4 k, K pass 26.7 k (319 KB per CU: the HBM rate), maxima 3.9 k, V pass 24.9 k, sums 9.3 k, output 1.3 k, scorer 20.3 k
// = 92.8 k cycles.  Built and rejected: all exponentials between the K pass and the V pass (a 11.3 k-cycle phase with the ring
// full and idle): 50.7-51.0 us.  0 spilled registers (249-251 VGPRs); the DMAs are inline asm because hipcc waits `vmcnt(0)` in front
// of every LDS access it cannot prove disjoint from a builtin DMA's destination (see ekr_dma16).
#include <algorithm>

#include "ekv_common.h"
#include "ekv_kernels.h"
#if EKV_BF16   // (bf16 instance: the same kernel under a tagged name)
#define ekv_attn_resident_kernel ekv_attn_resident_kernel_bf16
#endif

#define EKV_SS_NT 512
#define EKV_SS_DEVICE_ONLY
#include "ekv_score_select.inc"
#include "ekv_wide_tail.h"

namespace {

typedef float ekr_f16v __attribute__((ext_vector_type(16)));
typedef short ekr_s4 __attribute__((ext_vector_type(4)));
typedef float ekr_f4 __attribute__((ext_vector_type(4)));
typedef ekv_e ekr_h4 __attribute__((ext_vector_type(4)));

// (R_* and the two LDS layouts RL<LONG> of the kernel: ekv_geometry.h)

// 16 bytes per lane global -> LDS (global_load_lds_dwordx4): lds_dst = wave-uniform base of a 1 KB piece, lane i lands at + 16 * i.
// By inline asm (cdna_hip_programming.md §5.7: M0 written in the statement that reads it), NOT the builtin: hipcc models the builtin
// as an LDS store that every later LDS access may alias and puts `s_waitcnt vmcnt(0)` in front of the P^T writes and of the first
// transposing read of every tile of the V pass — the ring then holds ONE tile.  Hidden from it, the only waits are the counted ones
// below; nothing else of the stream loops touches vector memory (slot entries come from LDS).
// nt: non-temporal loads (MI355X_MICROARCH.md "nt-weights": issued -> landed -18 % on rows one CU reads once) for launches whose K + V
// exceed the Infinity Cache; a launch that fits it keeps the default policy — a chunked prefill re-reads the same bank every step, and
// with the rows left in the cache the configs[2] step measured 45.4-45.5 us against 46.8-47.0 us with nt (same box, alternating).
__device__ __forceinline__ void ekr_dma16(const char* src, char* lds_dst, const bool nt) {
  const uint32_t ldsa = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds_dst;
  unsigned keep;
  if (nt)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(ldsa) : "memory");
  else
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(ldsa) : "memory");
}
// LDS-DMAs stay in flight across these (a workgroup-scope fence would wait for them: they are LDS stores to it)
__device__ __forceinline__ void ekr_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void ekr_halves(float x, float& lo, float& hi) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  lo = __uint_as_float(r[0]);
  hi = __uint_as_float(r[1]);
}
// all-reduce over the 32 lanes of a half-wave (every lane gets the result): four DPP steps inside the 16-lane rows, one swizzle across
__device__ __forceinline__ float ekr_max32(float x) {
  x = fmaxf(x, ekv_dpp<0xB1>(x));
  x = fmaxf(x, ekv_dpp<0x4E>(x));
  x = fmaxf(x, ekv_dpp<0x141>(x));
  x = fmaxf(x, ekv_dpp<0x140>(x));
  return fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, x), 0x401F)));
}
__device__ __forceinline__ float ekr_sum32(float x) {
  x += ekv_dpp<0xB1>(x);
  x += ekv_dpp<0x4E>(x);
  x += ekv_dpp<0x141>(x);
  x += ekv_dpp<0x140>(x);
  return x + __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, x), 0x401F));
}

// REP: the GQA factor (1 / 2 / 4 / 8), a compile-time constant as in the column-sum pass of ekv_attn_wide.inc
template <int REP, bool LONG>
__global__ void __launch_bounds__(R_NT, 1) ekv_attn_resident_kernel(const EkvAttnArgs a, const EkvScoreArgs sc) {
  using Ly = RL<LONG>;
  constexpr int D = R_D, NT = R_NT, TK = R_TK, NB = R_NB, KS = D / 16, PPR = D / 8, RS = R_RS;
  constexpr int TILES = Ly::TILES, TMAX = Ly::TMAX, PSTR = Ly::PSTR, PBUF = Ly::PBUF, NSH = Ly::NSH;
  constexpr int LPT = 4, RPI = 4;                        // LDS-DMA instructions (1 KB = 4 rows each) per wave and tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const sP = smem + Ly::OFF_P;
  float* const sX = reinterpret_cast<float*>(smem + Ly::OFF_P);
  int32_t* const sSlot = reinterpret_cast<int32_t*>(smem + Ly::OFF_SLOT);
  float* const sCS = reinterpret_cast<float*>(smem + Ly::OFF_CS);
  float* const sM = reinterpret_cast<float*>(smem + Ly::OFF_RED);
  float* const sL = sM + 256;
  float* const sInv = sL + 256;

  const int n = a.q_len, T = a.n_slots, t_new = T - n;
  constexpr int rep = REP, rsh = REP == 1 ? 0 : (REP == 2 ? 1 : (REP == 4 ? 2 : 3));
  const int NR = rep * n;
  const int h = blockIdx.x, ll = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wq = wave & 1, wk = wave >> 1;
  const int rbase = LONG ? 0 : wq * 32;                  // first row of the block this wave holds
  const int sh = LONG ? wave : wk;                       // its share of a row's statistics
  const int hi = lane >> 5, c31 = lane & 31, G = lane >> 4, c = lane & 15;
  const int n_tiles = (T + TK - 1) / TK, n_items = 2 * n_tiles;      // stream items: K tiles, then V tiles
  const size_t head_row = ((size_t)(a.layer_begin + ll) * a.n_kv_heads + h) * a.cap;
  const int32_t* const slot_row = a.slot_of_pos + head_row;
  const float cexp = EKV_LOG2E * (1.f / a.sm_div);

  const char* const k_old = reinterpret_cast<const char*>(a.k + head_row * D);
  const char* const v_old = reinterpret_cast<const char*>(a.v + head_row * D);
  const char* const k_nw = reinterpret_cast<const char*>(a.k_new + (size_t)ll * a.n_kv_heads * n * D + (size_t)h * a.kv_hs);
  const char* const v_nw = reinterpret_cast<const char*>(a.v_new + (size_t)ll * a.n_kv_heads * n * D + (size_t)h * a.kv_hs);
  const uint32_t kvrs = (uint32_t)a.kv_ts * 2u;

#ifdef EKR_PROFILE      // cycle stamps per head in the (unused) tova_row scratch: tools/experiments/exp_resident_prof.py
  unsigned long long* const stamps = reinterpret_cast<unsigned long long*>(sc.tova_row) + ((size_t)ll * a.n_kv_heads + h) * 8;
#define EKR_STAMP(i) do { if (threadIdx.x == 0) stamps[i] = __builtin_readcyclecounter(); } while (0)
#else
#define EKR_STAMP(i) do { } while (0)
#endif
  EKR_STAMP(0);
  // ---- prologue: slot entries -> LDS, Q fragments -> registers (the chunk's own rows go to their cache slots behind the V pass) -------
  for (int j = tid; j < n_tiles * TK; j += NT) sSlot[j] = slot_row[max(min(j, t_new - 1), 0)];

  // Q operand ("query = lane": A of S = Q.K^T): row rbase + c31 of the block, d = 16*ks + 8*hi + [0, 8)
  ekv_h8 qreg[KS];
  {
    const int rowL = rbase + c31;
    const bool okL = rowL < NR;
    const int rL = okL ? rowL % rep : 0, iL = okL ? rowL / rep : 0;
    const char* const qb_ = reinterpret_cast<const char*>(a.q + (size_t)ll * a.n_q_heads * n * D + (size_t)(h * rep) * a.q_hs);
    const uint32_t qoff = (uint32_t)(rL * a.q_hs + iL * a.q_ts + 8 * hi) * 2u;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      qreg[ks] = *reinterpret_cast<const ekv_h8*>(qb_ + (qoff + 32u * ks));
      if (!okL) qreg[ks] = ekv_h8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qreg[ks]));      // (complete here: not sunk behind the first DMAs with a wait of its own)
  ekr_barrier();

  // ---- the stream: item u < n_tiles = K tile u, else V tile u - n_tiles, into ring slot u % NB ------------------------------------
  // instruction p of wave w fills the 1 KB piece w * LPT + p of the tile = rows row0 + p * RPI; the LDS image is lane-linear, so the
  // swizzle sits on the SOURCE address (ekv_attn_wide.inc: K chunk ^ (row & 15), V chunk ^ ((row & 3) << 2))
  const int row0 = wave * (LPT * RPI) + lane / PPR;
  const uint32_t k16 = (uint32_t)(((lane % PPR) ^ ((lane / PPR) & 15)) * 16);
  const uint32_t v16 = (uint32_t)(((lane % PPR) ^ (((lane / PPR) & 3) << 2)) * 16);
  const bool nt_loads = (size_t)gridDim.x * gridDim.z * (size_t)T * (2 * RS) > ((size_t)192 << 20);      // (workgroup-uniform)
  auto issue = [&](const int u) __attribute__((always_inline)) {
    const bool isv = u >= n_tiles;
    const int kt = (isv ? u - n_tiles : u) * TK;
    const char* const old_b = isv ? v_old : k_old;
    const char* const new_b = isv ? v_nw : k_nw;
    char* const dst = smem + (u % NB) * R_TBUF + wave * (LPT * 1024);
#pragma unroll
    for (int p = 0; p < LPT; ++p) {
      const int j = min(kt + row0 + p * RPI, T - 1);
      const bool is_new = j >= t_new;
      const uint32_t chunk = isv ? v16 : (k16 ^ (uint32_t)((p & 3) << 6));
      const uint32_t off_old = (uint32_t)sSlot[kt + row0 + p * RPI] * (uint32_t)RS + chunk;
      const uint32_t off_new = (uint32_t)(j - t_new) * kvrs + chunk;
      const char* const src = is_new ? new_b + off_new : old_b + off_old;
      ekr_dma16(src, dst + p * 1024, nt_loads);
    }
  };
  EKR_STAMP(1);
  issue(0);
  issue(1);

  // ---- 1. K pass: S of this wave's 32 rows x 32 keys of every tile ----------------------------------------------------------------
  ekr_f16v s[R_MAXT];
  const int ksw_l = c31 & 15;
#pragma unroll
  for (int b = 0; b < R_MAXT; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) s[b][r] = EKV_NEG_INF;
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    if (t < n_tiles) {                                  // (workgroup-uniform)
      if (t + 1 < n_items) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      ekr_barrier();
      if (t + 2 < n_items) issue(t + 2);
      if (LONG && (t & 1) != wq) continue;              // (wave-uniform: the other query-wave group's tile)
      const char* const kbase = smem + (t % NB) * R_TBUF + (wk * 32 + c31) * RS;
      ekr_f16v acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const ekv_h8 kf = *reinterpret_cast<const ekv_h8*>(kbase + (((2 * ks + hi) ^ ksw_l) << 4));
        acc = EKV_MFMA_32x32x16(qreg[ks], kf, acc, 0, 0, 0);      // S[q][key]
      }
      // register r <-> row rbase + (r&3) + 8*(r>>2) + 4*hi, key = lane.  Tiles that reach the chunk's own positions or the end of the
      // range take the causal / range mask: key j is visible to token i iff j <= t_new + i
      const int j = t * TK + wk * 32 + c31;
      if (t * TK + TK > t_new + 1) {
        const int jj = j >= T ? 0x7fffffff : j - (t_new + 1 + ((rbase + 4 * hi) >> rsh));
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (jj >= (((r & 3) + 8 * (r >> 2)) >> rsh)) acc[r] = EKV_NEG_INF;
      }
      s[LONG ? t >> 1 : t] = acc;
    }
  }

  EKR_STAMP(2);
  // ---- 2. exact row maxima over the resident logits -----------------------------------------------------------------------------
  float rowv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float mx = s[0][r];
#pragma unroll
    for (int t = 1; t < R_MAXT; ++t) mx = fmaxf(mx, s[t][r]);
    rowv[r] = ekr_max32(mx);
  }
  if (c31 == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) sM[(rbase + (r & 3) + 8 * (r >> 2) + 4 * hi) * NSH + sh] = rowv[r];
  }
  ekr_barrier();
  // (the shares of the waves that hold keys of a row are combined by one thread per row and handed out as one word per row — sixteen
  //  16-byte reads of the shares per lane were 64 live registers on top of the logits: spills)
  if (tid < 256 / NSH) {
    float mrow = sM[tid * NSH];
#pragma unroll
    for (int i = 1; i < NSH; ++i) mrow = fmaxf(mrow, sM[tid * NSH + i]);
    sInv[tid] = -(mrow * cexp);
  }
  ekr_barrier();
#pragma unroll
  for (int q4 = 0; q4 < 4; ++q4) {
    const ekr_f4 nm = *reinterpret_cast<const ekr_f4*>(sInv + rbase + 8 * q4 + 4 * hi);
#pragma unroll
    for (int e = 0; e < 4; ++e) rowv[4 * q4 + e] = nm[e];
  }
  float rows[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) rows[r] = 0.f;
  EKR_STAMP(3);
  // ---- 3. V pass: the exponentials of a tile, then O^T[d][q] of this wave's 32 d x 32 q block over all keys ----------------------------------------------------------
  ekr_f16v oacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) oacc[r] = 0.f;
  const int vsw_l = c >> 2;
  const int tr_lane = 32 * (G & 1) + 16 * ((c & 3) >> 1) + 8 * (c & 1);      // transposing reads: lane c supplies row (c >> 2), 8-byte piece (c & 3)
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    if (t < n_tiles) {
      const int u = n_tiles + t;
      if (!LONG || (t & 1) == wq) {                     // (wave-uniform) this wave holds logits of the tile
        const int b = LONG ? t >> 1 : t;                // (a constant after unrolling)
        // this wave's p' of the tile -> P^T[key][q]
        char* const pw = sP + (t & 1) * PBUF + (wk * 32 + c31) * PSTR + (rbase + 4 * hi) * 2;
        // p' of this tile NOW, under the wait for the stream (the V pass is bound by its DMAs; 16 exponentials per lane and tile)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[b][r], cexp, rowv[r]));
          s[b][r] = p;
          rows[r] += p;
        }
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
          *reinterpret_cast<ekr_h4*>(pw + 16 * q4) = ekr_h4{(ekv_e)s[b][4 * q4], (ekv_e)s[b][4 * q4 + 1], (ekv_e)s[b][4 * q4 + 2], (ekv_e)s[b][4 * q4 + 3]};
      }
      // (the P^T tile does not depend on the stream: written before the wait for the V tile)
      if (u + 1 < n_items) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      ekr_barrier();
      if (u + 2 < n_items) issue(u + 2);
      const char* const vb = smem + (u % NB) * R_TBUF + (4 * hi + (c >> 2)) * RS + tr_lane;
      const char* const pb = sP + (t & 1) * PBUF + (4 * hi + (c >> 2)) * PSTR + tr_lane + (LONG ? 0 : wq * 64);
      // (LONG: the two query-wave groups take the two halves of the tile's keys; their O^T blocks are added behind the loop)
      const int kb0 = LONG ? wq * 4 : 0;
#pragma unroll
      for (int kq = 0; kq < (LONG ? 4 : 8); ++kq) {      // 16 keys per MFMA: k-slots j < 4 <-> keys 16*kb + 4*hi + j, j >= 4 <-> 16*kb + 8 + 4*hi + (j - 4)
        const int kb = kb0 + kq;
        const char* const vp = vb + (16 * kb) * RS + ((wk ^ vsw_l) << 6);
        const char* const pp = pb + (16 * kb) * PSTR;
        const ekr_h4 v_lo = __builtin_bit_cast(ekr_h4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ekr_s4*)(vp)));
        const ekr_h4 v_hi = __builtin_bit_cast(ekr_h4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ekr_s4*)(vp + 8 * RS)));
        const ekr_h4 p_lo = __builtin_bit_cast(ekr_h4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ekr_s4*)(pp)));
        const ekr_h4 p_hi = __builtin_bit_cast(ekr_h4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ekr_s4*)(pp + 8 * PSTR)));
        const ekv_h8 aV = {v_lo[0], v_lo[1], v_lo[2], v_lo[3], v_hi[0], v_hi[1], v_hi[2], v_hi[3]};
        const ekv_h8 bP = {p_lo[0], p_lo[1], p_lo[2], p_lo[3], p_hi[0], p_hi[1], p_hi[2], p_hi[3]};
        oacc = EKV_MFMA_32x32x16(aV, bP, oacc, 0, 0, 0);
      }
    }
  }

  // The stream is over: from here on ordinary loads are free again.  Requested NOW, consumed behind the column-sum phase (one round trip
  // hidden): the chunk's own K / V rows for the append (L2-warm: the stream has just read them) and the score rows of the scorer.
  // (Nobody reads the new rows' cache slots in this launch: the stream takes them from k_new / v_new.)
  constexpr int APT = (64 * PPR + NT - 1) / NT, TI = Ly::TI;
  int a_slot[APT];
  ekv_u4 a_k[APT], a_v[APT];
  const int n_pieces = n * PPR;
#pragma unroll
  for (int u = 0; u < APT; ++u) {
    const int piece = min(tid + u * NT, n_pieces - 1);      // unconditional (clamped) loads
    a_slot[u] = slot_row[t_new + piece / PPR];
    const uint32_t po = (uint32_t)(piece / PPR) * kvrs + (uint32_t)(piece % PPR) * 16u;
    a_k[u] = *reinterpret_cast<const ekv_u4*>(k_nw + po);
    a_v[u] = *reinterpret_cast<const ekv_u4*>(v_nw + po);
  }
  float pS[TI], pQ[TI], pC[TI];
  ekw_tail_preload<TI>(sc, h, ll, pS, pQ, pC);
  EKR_STAMP(4);
  ekr_barrier();      // (every wave is through its last tiles: the exchange buffers below alias them)
  if (LONG) {
    // the two key halves of every tile: group 1's O^T block joins group 0's (16 floats per lane through the ring's memory)
    ekr_f4* const xo = reinterpret_cast<ekr_f4*>(smem) + (size_t)(wk * 64 + lane) * 4;
    if (wq == 1) {
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) xo[q4] = ekr_f4{oacc[4 * q4], oacc[4 * q4 + 1], oacc[4 * q4 + 2], oacc[4 * q4 + 3]};
    }
    ekr_barrier();
    if (wq == 0) {
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const ekr_f4 x = xo[q4];
#pragma unroll
        for (int e = 0; e < 4; ++e) oacc[4 * q4 + e] += x[e];
      }
    }
  }
  // ---- 4a. row sums: the waves' shares through LDS, 1 / L per row -------------------------------------------------------
  float inv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) rows[r] = ekr_sum32(rows[r]);
  if (c31 == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) sL[(rbase + (r & 3) + 8 * (r >> 2) + 4 * hi) * NSH + sh] = rows[r];
  }
  ekr_barrier();
  // 1 / L of the block's rows (0 for the rows past the block: they count nowhere)
  if (tid < 256 / NSH) {
    float L = sL[tid * NSH];
#pragma unroll
    for (int i = 1; i < NSH; ++i) L += sL[tid * NSH + i];      // (fixed order)
    sInv[tid] = tid < NR ? 1.f / L : 0.f;
  }
  ekr_barrier();
#pragma unroll
  for (int q4 = 0; q4 < 4; ++q4) {
    const ekr_f4 il = *reinterpret_cast<const ekr_f4*>(sInv + rbase + 8 * q4 + 4 * hi);
#pragma unroll
    for (int e = 0; e < 4; ++e) inv[4 * q4 + e] = il[e];
  }
  float part[R_MAXT];
  // ---- 4b. column sums of the GQA-folded probabilities (the arithmetic of ekv_attn_wide.inc's column-sum pass) ----------------------
#pragma unroll
  for (int b = 0; b < R_MAXT; ++b) {
    const int t = LONG ? 2 * b + wq : b;                // the tile of this wave's block b
    if (t < n_tiles) {
      float cs = 0.f, cq = 0.f;
      if (REP == 1) {
        ekv_f2 cs2 = {0.f, 0.f}, cq2 = {0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const ekv_f2 p2 = {s[b][r] * inv[r], s[b][r + 1] * inv[r + 1]};
          cs2 += p2;
          cq2 += p2 * p2;
        }
        cs = cs2.x + cs2.y;
        cq = cq2.x + cq2.y;
      } else if (REP == 2) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const float pb = (s[b][r] * inv[r] + s[b][r + 1] * inv[r + 1]) * 0.5f;
          cs += pb;
          cq += pb * pb;
        }
      } else if (REP == 4) {
#pragma unroll
        for (int r = 0; r < 16; r += 4) {
          const float pb = (((s[b][r] * inv[r] + s[b][r + 1] * inv[r + 1]) + s[b][r + 2] * inv[r + 2]) + s[b][r + 3] * inv[r + 3]) * 0.25f;
          cs += pb;
          cq += pb * pb;
        }
      } else {
        // GQA x 8: a query's heads span BOTH half-waves (rows 8g .. 8g+3 in the lower half, 8g+4 .. 8g+7 in the upper): the halves'
        // partial sums are exchanged and the lower half counts the query (ekv_attn_wide.inc's run-time fold)
#pragma unroll
        for (int r = 0; r < 16; r += 4) {
          const float part4 = ((s[b][r] * inv[r] + s[b][r + 1] * inv[r + 1]) + s[b][r + 2] * inv[r + 2]) + s[b][r + 3] * inv[r + 3];
          float l0, h0;
          ekr_halves(part4, l0, h0);
          const float pb = (l0 + h0) * 0.125f;
          if (hi == 0) {
            cs += pb;
            cq += pb * pb;
          }
        }
      }
      float clo, chi, qlo, qhi;
      ekr_halves(cs, clo, chi);
      ekr_halves(cq, qlo, qhi);
      const float mine = hi == 0 ? clo + chi : qlo + qhi;      // lower half-wave: sum, upper: sum of squares
      if (LONG) {
        sCS[hi * TMAX + t * TK + wk * 32 + c31] = mine;        // (this wave holds every row of the block: complete)
      } else {
        part[b] = mine;
        if (wq == 1) sX[hi * TMAX + t * TK + wk * 32 + c31] = mine;      // (query wave 0 adds the two shares in wave order)
      }
    }
  }
  ekr_barrier();
  if (!LONG) {
    if (wq == 0) {
#pragma unroll
      for (int t = 0; t < R_MAXT; ++t)
        if (t < n_tiles) {
          const int j = t * TK + wk * 32 + c31;
          sCS[hi * TMAX + j] = part[t] + sX[hi * TMAX + j];
        }
    }
    ekr_barrier();
  }
#pragma unroll
  for (int u = 0; u < APT; ++u) {
    const int piece = tid + u * NT;
    if (piece < n_pieces) {
      const size_t off = (head_row + a_slot[u]) * D;
      reinterpret_cast<ekv_u4*>(a.k_w + off)[piece % PPR] = a_k[u];
      reinterpret_cast<ekv_u4*>(a.v_w + off)[piece % PPR] = a_v[u];
    }
  }
  EKR_STAMP(5);
  // ---- 5. output: register r <-> d = wk*32 + (r&3) + 8*(r>>2) + 4*hi, query = lane -------------------------------------------------
  {
    const int rowE = rbase + c31;
    if (rowE < NR && (!LONG || wq == 0)) {
      const float il = sInv[rowE];
      __half* orow = a.out_direct + (size_t)ll * a.n_q_heads * n * D + (size_t)(h * rep + rowE % rep) * a.o_hs + (size_t)(rowE / rep) * a.o_ts;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const __half2 lo = ekv_to_e2(oacc[4 * q4] * il, oacc[4 * q4 + 1] * il);
        const __half2 hh = ekv_to_e2(oacc[4 * q4 + 2] * il, oacc[4 * q4 + 3] * il);
        uint2 pk;
        pk.x = __builtin_bit_cast(unsigned int, lo);
        pk.y = __builtin_bit_cast(unsigned int, hh);
        *reinterpret_cast<uint2*>(orow + wk * 32 + 8 * q4 + 4 * hi) = pk;
      }
    }
  }

  // ---- 6. the scorer of this head (ekv_wide_tail.h): accumulate, select, compact — keys and scratch in the ring's memory ------------
  __syncthreads();
  EKR_STAMP(6);
  ekw_score_tail<TI>(sc, h, ll, smem, sCS, sCS + TMAX, pS, pQ, pC);
  EKR_STAMP(7);
}

template <int REP, bool LONG>
hipError_t launch_resident(const EkvAttnArgs& a, const EkvScoreArgs& sc, int layer_count, hipStream_t s) {
  auto* fn = &ekv_attn_resident_kernel<REP, LONG>;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, RL<LONG>::LDS);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL(fn, dim3(a.n_kv_heads, 1, layer_count), dim3(R_NT), RL<LONG>::LDS, s, a, sc);
  return hipGetLastError();
}
template <int REP>
hipError_t launch_resident_rep(const EkvAttnArgs& a, const EkvScoreArgs& sc, int layer_count, hipStream_t s) {
  // (query blocks of <= 32 rows fit both shapes up to 1280 keys and take the short one — measured, us per step short / LONG: 32 rows x
  //  1240 keys, 256 heads 44.1 / 45.4; 16 rows 43.3 / 45.4; 32 rows x 1088 keys, 1024 heads 176-180 / 175-177.  A/B switch:
  //  EKV_RESIDENT_LONG_MIN_T = first key count that takes the LONG shape)
  static const int long_min_t = [] { const char* e = std::getenv("EKV_RESIDENT_LONG_MIN_T"); return e != nullptr ? std::atoi(e) : RL<false>::TMAX + 1; }();
  const bool lng = a.n_slots > RL<false>::TMAX || ((a.n_q_heads / a.n_kv_heads) * a.q_len <= 32 && a.n_slots >= long_min_t);
  return lng ? launch_resident<REP, true>(a, sc, layer_count, s) : launch_resident<REP, false>(a, sc, layer_count, s);
}

hipError_t launch_resident_any(const EkvAttnArgs& a, const EkvScoreArgs& sc, int layer_count, hipStream_t s) {
  if (a.out_direct == nullptr) return hipErrorInvalidValue;
  switch (a.n_q_heads / a.n_kv_heads) {
    case 1: return launch_resident_rep<1>(a, sc, layer_count, s);
    case 2: return launch_resident_rep<2>(a, sc, layer_count, s);
    case 4: return launch_resident_rep<4>(a, sc, layer_count, s);
    case 8: return launch_resident_rep<8>(a, sc, layer_count, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t EKV_FN_D_ELEM(ekv_launch_attn_resident, 128, EKV_ELEM)(const EkvAttnArgs& a, const EkvScoreArgs& sc, int layer_count, hipStream_t s) {
  return launch_resident_any(a, sc, layer_count, s);
}
