// ekv_chunk8_kernel: a chunk step (q_len = n > 1: strided-prefill chunks and the dense prefix) over FP8 code rows ("kv8 chunks",
// include/easykv_hip.h; the ekv_kv8_chunk_* calls), MFMA 16x16x32 f16 / bf16.  Compiled once per (EKV_D = 64 | 128, element type) by the
// EKV_CHUNK_CODES lines of the manifest; launch code in ekv_attn_chunk8.hip.  Plain keys, one pass with online softmax, raw logits exported
// for the scorer, blocks of at most 32 GQA-folded rows (ekv_chunk_blocks(..., kChunkNarrowD): larger q_len = several blocks; GQA factors
// above 32 are refused by the planner).  No two-pass, wide, logits-in-LDS or logits-resident form.
//
// Work split: the 16-bit one-tile kernel's (ekv_attn_chunk.inc, QPW = 1, NW = 4), so that the (m, l, o) partials, the in-kernel fold, the
// row statistics, the exported logits and the scorer behind or inside the launch are the 16-bit step's.  One workgroup of 4 waves per
// (key-range split x query block, KV head, layer); wave (wk, wq) owns 32 of the 64 keys of a super-tile and the 16-row query tile wq.
//
// Staging.  A lane's 16-byte load is 16 codes: a head_dim-128 row is 8 lanes, a head_dim-64 row 4, and a 64-position super-tile is
// 64 * D bytes per tensor — 2 (D 128) or 1 (D 64) pieces per thread, half the staging registers of the 16-bit kernel.  Rows are gathered
// through the slot map; the fp32 row scales, indexed by PHYSICAL row, are gathered with them (by the lane that holds a row's first piece).  The loads of tile t + 1 are issued once tile t is in LDS and fly while it is consumed.
//   Where the codes are widened: BEFORE the LDS store.  The MFMA side then sees the 16-bit operand layouts unchanged — K rows as
//   ds_read_b128 A operands, V through the transposing ds_read_b64_tr_b16 — and widening costs 8 (K) + 8 (V) conversions per piece
//   once per tile, not once per query wave.  Widening after the LDS read would halve the LDS of a tile (9 KB instead of 18 KB per tensor
//   at head_dim 128) and allow twice the tiles in flight, but the transposing read has no 8-bit form that lands in the f16 MFMA's operand
//   layout, so V would be gathered byte-wise (16 ds_read_u8 per d-block and lane) and both query waves would widen the same K rows.  This
//   kernel is HBM-bound with one tile in flight per workgroup and two workgroups per CU; its LDS is the 16-bit one-tile build's plus 512
//   bytes of row scales (ekv_chunk8_lds, ekv_geometry.h), its VGPRs are below (profiles/kv8_chunk_registers.txt).
// K side.  Widening a code to f16 / bf16 is exact (v_cvt_scalef32_pk_{f16,bf16}_fp8, scale 1).  S^T = K . Q^T on the widened codes; the
//   accumulator rows are keys, so each element is multiplied in fp32 by k_scale of its key (read from the tile's scale row in LDS) and then
//   divided by sm_div (correctly rounded): logit = (q . codes) * k_scale[row] / sm_div, the decode stream's operations in its order.
// V side.  v_scale[row] reaches O^T += V^T . P^T through P: V is widened exactly, p * v_scale[key] is formed in fp32 and split into a
//   16-bit pair hi + lo (two PV MFMAs per d-block; the kernel is HBM-bound and the MFMA pipe has the room), so neither fp16's subnormal
//   range nor a second rounding of V touches the output.  Two alternatives were built and measured, then removed: V scaled as it is widened
//   (one more rounding per element) and the scale folded into a single 16-bit P.
//   Largest |out - float64 reference| over the cases of tests/test_hip_kv8_chunk.py, fp16 / bf16: hi + lo P 1.29e-3 / 4.9e-4, scaled V
//   1.78e-3 / 9.0e-4, single P 3.12e-3 / 1.22e-3 (28 of 48 cases miss the output bar); DESIGN.md §8 "chunk steps on FP8 rows".
// Appended rows.  The chunk's n new K/V rows arrive 16-bit in k_new / v_new.  Every workgroup quantises the new rows IT attends in
//   registers as it stages them (two 16-byte loads per piece, row maximum over the row's lane group, s = amax / 448 or 1, code = RNE(x / s)
//   from the correctly rounded quotient: ekv_fp8_row_scale / ekv_fp8_quant4, the conversion kernel's helpers) and widens the CODES, so new
//   rows are attended as quantised, causal mask included.  Exactly ONE workgroup stores a row's codes and scales: the (split, query block)
//   whose query block holds the row's own query and whose key range holds its position — the 16-bit kernel's append rule — in a prologue
//   that quantises by the same helpers (same bits).  Nobody reads those rows from the planes in this launch, so there is no race.
// No scalar memory writes; every store is a vector store.
#include <algorithm>
#include <type_traits>

#include "ekv_common.h"
#include "ekv_kernels.h"

#if EKV_BF16
#define ekv_chunk8_kernel ekv_chunk8_kernel_bf16
#endif

// FUSE: an unsplit one-block head's scorer runs as the tail of the workgroup that streamed the head (ekv_score_select_kernel's body, 256 threads)
#define EKV_SS_NT 256
#define EKV_SS_DEVICE_ONLY
#include "ekv_score_select.inc"

namespace {

typedef float ekv_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float ekv_max3(float x, float y, float z) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z));
  return r;
}

constexpr int kKT = kChunkKT;      // positions per super-tile
constexpr int kPadH = kChunkPadH;  // LDS row padding in 16-bit elements

// 16 elements of a 16-bit row (two 16-byte pieces) -> their 16 codes under the row's scale.  The PPR lanes that hold the row (an aligned
// lane group) agree on the maximum; every lane of the group must be active.
template <int PPR>
__device__ __forceinline__ uint4 ekv_chunk8_quant16(const uint4& x0, const uint4& x1, float* scale) {
  float f[16];
  const float m = fmaxf(ekv_widen8_amax(x0, f), ekv_widen8_amax(x1, f + 8));
  const float s = ekv_fp8_row_scale(ekv_group_max<PPR>(m));
  *scale = s;
  return uint4{ekv_fp8_quant4(f[0], f[1], f[2], f[3], s), ekv_fp8_quant4(f[4], f[5], f[6], f[7], s),
               ekv_fp8_quant4(f[8], f[9], f[10], f[11], s), ekv_fp8_quant4(f[12], f[13], f[14], f[15], s)};
}
// 4 codes -> 4 elements, exact
__device__ __forceinline__ void ekv_chunk8_widen4(uint32_t w, ekv_e* e) {
  const ekv_h2 lo = ekv_fp8_pk_e<false>(w), hi = ekv_fp8_pk_e<true>(w);
  e[0] = lo[0], e[1] = lo[1], e[2] = hi[0], e[3] = hi[1];
}
// 16 codes -> 16 elements, exact
__device__ __forceinline__ void ekv_chunk8_widen16(const uint4& c, ekv_h8* h0, ekv_h8* h1) {
  ekv_e e[16];
  ekv_chunk8_widen4(c.x, e), ekv_chunk8_widen4(c.y, e + 4), ekv_chunk8_widen4(c.z, e + 8), ekv_chunk8_widen4(c.w, e + 12);
  *h0 = ekv_h8{e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7]};
  *h1 = ekv_h8{e[8], e[9], e[10], e[11], e[12], e[13], e[14], e[15]};
}

template <bool FUSE>
__global__ void __launch_bounds__(256, 2) ekv_chunk8_kernel(const EkvAttnArgs a, const EkvScoreArgs sc) {
  constexpr int D = EKV_D;
  constexpr int NT = 256;
  constexpr int PPR = D / kChunk8EPL;       // 16-byte pieces per code row: 8 or 4
  constexpr int LPT = kKT * PPR / NT;       // pieces per thread per tensor per super-tile: 2 or 1
  constexpr int RS = D + kPadH;             // LDS row stride (16-bit elements)
  constexpr int KB = D / 32;                // MFMA k-steps of QK^T
  constexpr int DB = D / 16;                // d-blocks of O^T
  constexpr int PS = D + 2;
  static_assert(D == 64 || D == 128, "FP8 rows: head_dim 64 and 128");
  static_assert(LPT * NT == kKT * PPR, "whole pieces per thread");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int32_t* s_slot = reinterpret_cast<int32_t*>(smem);
  ekv_e* sK = reinterpret_cast<ekv_e*>(smem + ekv_align((size_t)a.rows_per_split * 4, 16));
  ekv_e* sV = sK + kKT * RS;
  float* s_ks = reinterpret_cast<float*>(sV + kKT * RS);      // k_scale of the tile's 64 rows
  float* s_vs = s_ks + kKT;                                    // v_scale of the same rows

  const int n = a.q_len, T = a.n_slots;
  const int rep = a.n_q_heads / a.n_kv_heads;
  // (heads fastest, query blocks in descending order: the 16-bit kernel's grid)
  const int qb = a.n_qblocks - 1 - (int)(blockIdx.y % a.n_qblocks), split = blockIdx.y / a.n_qblocks;
  const int h = blockIdx.x, ll = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int wk = wave & 1, wq = wave >> 1;
  const int i0 = qb * a.qb_rows, nb = min(a.qb_rows, n - i0);   // queries [i0, i0 + nb) of the chunk
  const int NR = rep * nb;                                      // rows of this block: row = (i - i0) * rep + r
  const int t0 = split * a.rows_per_split;
  const int t1 = min(min(T, t0 + a.rows_per_split), T - n + i0 + nb);   // causal bound of the block
  const size_t head_row = ((size_t)(a.layer_begin + ll) * a.n_kv_heads + h) * a.cap;
  const int t_new = T - n;                                      // first position of the chunk itself
  const int nse = a.n_split * 2;
  const float inv_sm_div = 1.f / a.sm_div;
  constexpr float kMFloor = -1.0e30f;

  for (int i = tid; i < t1 - t0; i += NT) s_slot[i] = a.slot_of_pos[head_row + t0 + i];
  __syncthreads();

  // per-wave state: ONE query tile
  ekv_f4 oacc[DB];
  const int row = wq * 16 + c;
  const bool row_ok = row < NR;
  const int row_r = row_ok ? row % rep : 0;        // the rep query heads of one query sit in adjacent lanes
  const int row_i = row_ok ? i0 + row / rep : i0;
  float m_run = EKV_NEG_INF, l_run = 0.f;
#pragma unroll
  for (int db = 0; db < DB; ++db) oacc[db] = ekv_f4{0.f, 0.f, 0.f, 0.f};

  // bases: the code planes of this head (one byte per element), this launch's new rows of this head (16-bit)
  const char* const k_old = reinterpret_cast<const char*>(a.k) + head_row * D;
  const char* const v_old = reinterpret_cast<const char*>(a.v) + head_row * D;
  const char* const k_nw = reinterpret_cast<const char*>(a.k_new + (size_t)ll * a.n_kv_heads * n * D + (size_t)h * a.kv_hs);
  const char* const v_nw = reinterpret_cast<const char*>(a.v_new + (size_t)ll * a.n_kv_heads * n * D + (size_t)h * a.kv_hs);
  const uint32_t kvrs = (uint32_t)a.kv_ts * 2u;      // bytes between two of this launch's new rows

  // ---- append: the (split, query block) that owns the new positions [t_new + i0, t_new + i0 + nb) within its key range quantises their
  // rows and stores codes + scales into the rows the slot map names.  Whole lane groups run every iteration (the row maximum is a group
  // reduction); a group past the end works on the first row and stores nothing.
  {
    const int j_lo = max(t_new + i0, t0), j_hi = min(t_new + i0 + nb, t1);
    const int n_pieces = max(j_hi - j_lo, 0) * PPR;
    for (int base = 0; base < n_pieces; base += NT) {
      const bool live = base + tid < n_pieces;
      const int piece = live ? base + tid : tid % PPR;
      const int j = j_lo + piece / PPR, sub = piece % PPR;
      const uint32_t noff = (uint32_t)(j - t_new) * kvrs + (uint32_t)sub * 32u;
      const uint4 k0 = *reinterpret_cast<const uint4*>(k_nw + noff), k1 = *reinterpret_cast<const uint4*>(k_nw + noff + 16);
      const uint4 v0 = *reinterpret_cast<const uint4*>(v_nw + noff), v1 = *reinterpret_cast<const uint4*>(v_nw + noff + 16);
      float sk, sv;
      const uint4 kc = ekv_chunk8_quant16<PPR>(k0, k1, &sk), vc = ekv_chunk8_quant16<PPR>(v0, v1, &sv);
      if (live) {
        const size_t prow = head_row + s_slot[j - t0];
        reinterpret_cast<uint4*>(reinterpret_cast<char*>(a.k_w) + prow * D)[sub] = kc;
        reinterpret_cast<uint4*>(reinterpret_cast<char*>(a.v_w) + prow * D)[sub] = vc;
        if (sub == 0) {
          a.k_scale[prow] = sk;
          a.v_scale[prow] = sv;
        }
      }
    }
  }

  // Q operands of this lane's query row, loaded once
  ekv_h8 qreg[KB];
  {
    const size_t qsrc = (size_t)ll * a.n_q_heads * n * D + (size_t)(h * rep + row_r) * a.q_hs + (size_t)row_i * a.q_ts;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      qreg[kb] = __builtin_bit_cast(ekv_h8, reinterpret_cast<const uint4*>(a.q + qsrc + kb * 32)[g]);
      if (!row_ok) qreg[kb] = ekv_h8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  // ---- staging: registers -> (quantise new rows) -> widen -> LDS ------------------------------------------------------------------------
  // c*: the 16 codes of a cache row's piece, or the first 8 elements of a new row's; n*: the second 8 elements of a new row's piece
  uint4 cK[LPT], cV[LPT], nK[LPT], nV[LPT];
  float ksl[LPT], vsl[LPT];
  // a tile that reaches the chunk's own rows or the end of the range (workgroup-uniform): its rows are clamped to the range and told apart
  auto tile_mixed = [&](int kt) { return kt + kKT > min(t_new, t1); };
  auto stage_load = [&](int kt) {
    const bool mixed = tile_mixed(kt);
#pragma unroll
    for (int p = 0; p < LPT; ++p) {
      const int piece = tid + p * NT;
      const int r = piece / PPR, sub = piece % PPR;
      const int j = mixed ? min(kt + r, t1 - 1) : kt + r;
      const bool is_new = mixed && j >= t_new;
      const int sl = is_new ? 0 : s_slot[j - t0];
      const char* const kp = is_new ? k_nw + ((uint32_t)(j - t_new) * kvrs + (uint32_t)sub * 32u) : k_old + ((uint32_t)sl * (uint32_t)D + (uint32_t)sub * 16u);
      const ptrdiff_t v_minus_k = is_new ? v_nw - k_nw : v_old - k_old;
      cK[p] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(kp)));
      cV[p] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(kp + v_minus_k)));
      nK[p] = nV[p] = uint4{0, 0, 0, 0};
      ksl[p] = vsl[p] = 1.f;
      if (is_new) {
        nK[p] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(kp + 16)));
        nV[p] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(kp + 16 + v_minus_k)));
      } else {
        if (sub == 0) ksl[p] = a.k_scale[head_row + sl];
        if (sub == 0) vsl[p] = a.v_scale[head_row + sl];
      }
    }
  };
  auto stage_store = [&](int kt) {
    const bool mixed = tile_mixed(kt);
#pragma unroll
    for (int p = 0; p < LPT; ++p) {
      const int piece = tid + p * NT;
      const int r = piece / PPR, sub = piece % PPR;
      uint4 kc = cK[p], vc = cV[p];
      float ks = ksl[p], vs = vsl[p];
      if (mixed) {      // (workgroup-uniform: the group reductions run in every lane; the lanes of a cache row discard what they computed)
        float ksn, vsn;
        const uint4 kq = ekv_chunk8_quant16<PPR>(cK[p], nK[p], &ksn), vq = ekv_chunk8_quant16<PPR>(cV[p], nV[p], &vsn);
        if (min(kt + r, t1 - 1) >= t_new) kc = kq, vc = vq, ks = ksn, vs = vsn;
      }
      ekv_h8 h0, h1;
      ekv_chunk8_widen16(kc, &h0, &h1);
      *reinterpret_cast<ekv_h8*>(sK + r * RS + sub * 16) = h0;
      *reinterpret_cast<ekv_h8*>(sK + r * RS + sub * 16 + 8) = h1;
      ekv_chunk8_widen16(vc, &h0, &h1);
      *reinterpret_cast<ekv_h8*>(sV + r * RS + sub * 16) = h0;
      *reinterpret_cast<ekv_h8*>(sV + r * RS + sub * 16 + 8) = h1;
      if (sub == 0) {
        s_ks[r] = ks;
        s_vs[r] = vs;
      }
    }
  };

  // consume(kt): everything between the two barriers of one super-tile
  auto consume = [&](int kt) {
    const int kg = wk * 32;   // this wave's 32 keys of the super-tile
    if (kt + kg >= t1 || wq * 16 >= NR) return;      // (wave-uniform)
    // ---- S^T = K . Q^T on the widened codes: two 16-key tiles x the wave's query tile
    ekv_f4 S0 = {0.f, 0.f, 0.f, 0.f}, S1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const ekv_h8 a0 = *reinterpret_cast<const ekv_h8*>(sK + (kg + c) * RS + kb * 32 + g * 8);
      const ekv_h8 a1 = *reinterpret_cast<const ekv_h8*>(sK + (kg + 16 + c) * RS + kb * 32 + g * 8);
      S0 = EKV_MFMA_16x16x32(a0, qreg[kb], S0, 0, 0, 0);
      S1 = EKV_MFMA_16x16x32(a1, qreg[kb], S1, 0, 0, 0);
    }
    // accumulator slot e < 4 -> key 4g + e, e >= 4 -> key 16 + 4g + (e - 4): the row scales of those keys
    const float4 ks0 = *reinterpret_cast<const float4*>(s_ks + kg + 4 * g), ks1 = *reinterpret_cast<const float4*>(s_ks + kg + 16 + 4 * g);
    const float ksv[8] = {ks0.x, ks0.y, ks0.z, ks0.w, ks1.x, ks1.y, ks1.z, ks1.w};
    float sv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      // logit = (q . codes) * k_scale[row] / sm_div: the product rounded, then the correctly rounded quotient (reciprocal multiply + one
      // residual correction, as the 16-bit kernel divides)
      const float x = (e < 4 ? S0[e] : S1[e - 4]) * ksv[e];
      const float q0 = x * inv_sm_div;
      sv[e] = fmaf(fmaf(-a.sm_div, q0, x), inv_sm_div, q0);
    }
    // causal mask / end of the range, only where the wave's 32 keys reach them (wave-uniform test)
    if (kt + kg + 32 > min(t1, t_new + i0 + 1)) {
      const int jlim = min(t1, t_new + row_i + 1);   // first masked position for this query
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = kt + kg + (e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4));
        if (j >= jlim) sv[e] = EKV_NEG_INF;
      }
    }
    float mx = ekv_max3(ekv_max3(ekv_max3(sv[0], sv[1], sv[2]), sv[3], sv[4]), ekv_max3(sv[5], sv[6], sv[7]), EKV_NEG_INF);
    if (a.logits != nullptr && row_ok) {
      // each lane holds 4 consecutive keys per 16-key tile: two 16-byte stores (t_pad covers whole super-tiles; positions >= T receive -inf)
      float* lrow = a.logits + (((size_t)ll * a.n_q_heads + h * rep + row_r) * n + row_i) * a.t_pad + kt + kg + 4 * g;
      *reinterpret_cast<float4*>(lrow) = make_float4(sv[0], sv[1], sv[2], sv[3]);
      *reinterpret_cast<float4*>(lrow + 16) = make_float4(sv[4], sv[5], sv[6], sv[7]);
    }
    // ---- online softmax; the 4 lane groups of a query share the running maximum
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(fmaxf(m_run, mx), kMFloor);
    const float alpha = __builtin_amdgcn_exp2f((m_run - mn) * EKV_LOG2E);
    const float nm = -mn * EKV_LOG2E;
    const float4 v0 = *reinterpret_cast<const float4*>(s_vs + kg + 4 * g), v1 = *reinterpret_cast<const float4*>(s_vs + kg + 16 + 4 * g);
    const float vsv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    ekv_h8 bP = {0, 0, 0, 0, 0, 0, 0, 0}, bPl = {0, 0, 0, 0, 0, 0, 0, 0};
    float ls = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float p = __builtin_amdgcn_exp2f(fmaf(sv[e], EKV_LOG2E, nm));
      ls += p;
      const float pv = p * vsv[e];      // (p carries the key's V scale; hi + lo keep 22 bits of it)
      bP[e] = (ekv_e)pv;
      bPl[e] = (ekv_e)(pv - (float)bP[e]);
    }
    l_run = l_run * alpha + ls;
    m_run = mn;
    // ---- O^T = O^T * alpha + V^T . P^T (the rescale is skipped, wave-uniformly, while no lane's maximum moves)
    if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0ull) {
      asm volatile("" ::: "memory");
#pragma unroll
      for (int db = 0; db < DB; ++db) oacc[db] = oacc[db] * alpha;
    }
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      // two transposing LDS reads: the 16 lanes of group g fetch the 4-key x 16-column block of rows 4g .. 4g + 3, lane c receives column c
      typedef short ekv_s4 __attribute__((ext_vector_type(4)));
      typedef ekv_e ekv_h4 __attribute__((ext_vector_type(4)));
      const ekv_e* vp = sV + (kg + 4 * g + (c >> 2)) * RS + db * 16 + 4 * (c & 3);
      const ekv_h4 v_lo = __builtin_bit_cast(ekv_h4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ekv_s4*)vp));
      const ekv_h4 v_hi = __builtin_bit_cast(ekv_h4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ekv_s4*)(vp + 16 * RS)));
      const ekv_h8 aV = {v_lo[0], v_lo[1], v_lo[2], v_lo[3], v_hi[0], v_hi[1], v_hi[2], v_hi[3]};
      oacc[db] = EKV_MFMA_16x16x32(aV, bP, oacc[db], 0, 0, 0);
      oacc[db] = EKV_MFMA_16x16x32(aV, bPl, oacc[db], 0, 0, 0);
    }
  };

  if (t0 < t1) stage_load(t0);
  for (int kt = t0; kt < t1; kt += kKT) {
    ekv_lds_barrier();        // previous tile fully consumed
    stage_store(kt);
    ekv_lds_barrier();
    if (kt + kKT < t1) stage_load(kt + kKT);   // in flight while this tile is consumed
    consume(kt);
  }

  if (m_run <= kMFloor) m_run = EKV_NEG_INF;      // -inf = "no key seen"

  // ---- logits beyond this block's causal bound: the scorer reads every row over all T positions
  if (a.logits != nullptr) {
    const int t_end = min(T, t0 + a.rows_per_split);
    const int fill_lo = t0 < t1 ? t0 + (t1 - t0 + 31) / 32 * 32 : t0;   // consume() works in 32-key halves
    const int w = t_end - fill_lo;
    if (w > 0) {
      for (int idx = tid; idx < NR * w; idx += NT) {
        const int rw = idx / w, j = fill_lo + idx % w;
        a.logits[(((size_t)ll * a.n_q_heads + h * rep + rw % rep) * n + i0 + rw / rep) * a.t_pad + j] = EKV_NEG_INF;
      }
    }
  }

  float l = l_run;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);

  // ---- unsplit heads: fold the two key halves right here, write the output and the row statistics ---------------------------------------
  if (a.out_direct != nullptr) {
    constexpr int XS = DB * 4 + 2;                       // floats per lane: (m, l, o[DB][4])
    float* xch = reinterpret_cast<float*>(sK);           // the K/V tile buffers are free now (ekv_geometry.h)
    ekv_lds_barrier();
    float* mine = xch + (size_t)(wq * 64 + lane) * XS;
    if (wk == 1) {
      mine[0] = m_run;
      mine[1] = l;
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int e = 0; e < 4; ++e) mine[2 + db * 4 + e] = oacc[db][e];
    }
    ekv_lds_barrier();
    if (wk == 0 && row_ok) {
      const float m1 = mine[0], l1 = mine[1];
      const float mm = fmaxf(m_run, m1);
      const float w0 = m_run == EKV_NEG_INF ? 0.f : exp2f((m_run - mm) * EKV_LOG2E);
      const float w1 = m1 == EKV_NEG_INF ? 0.f : exp2f((m1 - mm) * EKV_LOG2E);
      const float lsum = l * w0 + l1 * w1;
      const float inv = 1.f / lsum;
      if (a.row_stats != nullptr && g == 0) {   // final softmax statistics of the row, for the scorer
        float* rs = a.row_stats + (((size_t)ll * a.n_q_heads + h * rep + row_r) * n + row_i) * 2;
        rs[0] = mm;
        rs[1] = lsum;
      }
      __half* orow = a.out_direct + (size_t)ll * a.n_q_heads * n * D + (size_t)(h * rep + row_r) * a.o_hs + (size_t)row_i * a.o_ts;
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        const __half2 lo = ekv_to_e2((oacc[db][0] * w0 + mine[2 + db * 4 + 0] * w1) * inv, (oacc[db][1] * w0 + mine[2 + db * 4 + 1] * w1) * inv);
        const __half2 hi = ekv_to_e2((oacc[db][2] * w0 + mine[2 + db * 4 + 2] * w1) * inv, (oacc[db][3] * w0 + mine[2 + db * 4 + 3] * w1) * inv);
        uint2 pk;
        pk.x = __builtin_bit_cast(unsigned int, lo);
        pk.y = __builtin_bit_cast(unsigned int, hi);
        *reinterpret_cast<uint2*>(orow + db * 16 + 4 * g) = pk;
      }
    }
    if (FUSE) {
      // Scorer tail.  This workgroup wrote every logit, the row statistics and the new rows of the head itself; the barrier makes them
      // visible to all of its waves.  Tiles, slot entries and scales in LDS are dead: the scorer's arrays take their place.
      __syncthreads();
      ekv_score_select_body(sc, h, ll, smem);
    }
    return;
  }

  // ---- partials: one per (split, wk), the 16-bit kernel's layout
  if (!row_ok) return;
  const size_t prow = (((size_t)ll * a.n_q_heads + h * rep + row_r) * n + row_i) * nse + split * 2 + wk;
  float* dst = a.partials + prow * PS;
  if (g == 0) {
    dst[0] = m_run;
    dst[1] = l;
  }
#pragma unroll
  for (int db = 0; db < DB; ++db) {
    float* o = dst + 2 + db * 16 + 4 * g;
    o[0] = oacc[db][0];
    o[1] = oacc[db][1];
    o[2] = oacc[db][2];
    o[3] = oacc[db][3];
  }
}

hipError_t launch8(const EkvAttnArgs& a, int layer_count, hipStream_t s, const EkvScoreArgs* fuse_sc) {
  size_t lds = ekv_chunk8_lds(EKV_D, a.rows_per_split);
  const dim3 grid(a.n_kv_heads, a.n_split * a.n_qblocks, layer_count);
  if (fuse_sc != nullptr) {
    if (a.n_split != 1 || a.n_qblocks != 1 || a.out_direct == nullptr) return hipErrorInvalidValue;
    lds = std::max(lds, ekv_score_lds_bytes(256, *fuse_sc));
    if (lds > 48 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_chunk8_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((ekv_chunk8_kernel<true>), grid, dim3(256), lds, s, a, *fuse_sc);
    return hipGetLastError();
  }
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_chunk8_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((ekv_chunk8_kernel<false>), grid, dim3(256), lds, s, a, EkvScoreArgs{});
  return hipGetLastError();
}

}  // namespace

hipError_t EKV_FN_D_ELEM(ekv_launch_attn_chunk8, EKV_D, EKV_ELEM)(const EkvAttnArgs& a, int layer_count, hipStream_t s, const EkvScoreArgs* fuse_sc) {
  static_assert(kKT == 64, "the accumulator-to-key map of consume() is a 64-position super-tile's");
  if (a.rope_cos != nullptr || a.k_scale == nullptr || a.v_scale == nullptr || a.q_len < 2 || (a.rows_per_split & 63) != 0) return hipErrorInvalidValue;
  return launch8(a, layer_count, s, fuse_sc);
}
