// ekv_attn_decode_g8_kernel: the split-path decode kernel for FP8 rows at GQA factors up to 16 ("kv8 gqa", include/easykv_hip.h; the
// ekv_kv8_gqa_* calls), MFMA 16x16x32.  head_dim EKV_D = 64 / 128, plain keys; compiled once per (element type, head_dim) by the
// EKV_DECODE_G8 lines of the manifest, launch code in ekv_attn_decode_g8.hip.  It keeps the contract of ekv_attn_decode_kernel
// (ekv_attn_decode.inc): fp32 logits to a.logits, (m, l, o[D]) partials per query head and split to a.partials, the appended row
// quantised and stored once, the optional last-arriver fold over a.arrive — so the fold, both scorers and the range compaction behind it
// are the 16-bit instances.
//
// Why it exists.  The VALU stream of FP8 rows (ekv_decode_stream.h, EPL = 16) gives each lane a 16-element piece of a row and a 16-float
// output slice PER QUERY HEAD: the GQA x 5 .. 8 builds spill, and a factor above 8 walks the rows twice.  Here the query heads of a KV
// head are the 16 columns of one MFMA tile (the work split of ekv_attn_decode_mxg.inc, the kernel for MXFP4 rows): 16 heads cost what
// one costs, and a wave's whole D x 16 output is D / 4 accumulator registers.
//
// Work split.  One workgroup of 4 waves per (key-range split, KV head, layer), no query-head-group factor.  The slot entries of the range
// are staged in LDS once.  Wave w takes the 32-key tiles w, w + 4, ... of the range on its own, without a workgroup barrier: it has its own
// V tile, scale words and online (m, l, o) state; the loads of its next tile fly while it consumes the current one.  Lane (g = lane / 16,
// c = lane % 16).
//
// Logits.  S^T[16 keys x 16 heads] per 16-key tile, two tiles (A: keys 0..15, B: 16..31) per step.  A row has ONE scale, constant along
// the MFMA's k-dimension, so (unlike the MXFP4 kernel's per-block products) all NK = D / 32 MFMAs of a tile run into one accumulator and
// the order of the elements along k is free as long as Q follows it: lane (g, c) takes the D / 4 CONTIGUOUS bytes g * D / 4 .. of key c —
// 32 bytes (two 16-byte loads) at head_dim 128, 16 bytes (one) at 64 — and MFMA i consumes bytes 8 i .. 8 i + 7 of them.  Q is the B
// operand, loaded once in the same order: lane (g, c) holds elements g * D / 4 + 8 i .. + 7 of head c for MFMA i, zeros for c >= rep
// (padded columns are never stored).  The codes are widened to the element type with scale 1 (v_cvt_scalef32_pk_{f16,bf16}_fp8: exact,
// e4m3 has 3 mantissa bits), and logit = acc * k_scale[row] / sm_div in fp32 — the FP8 stream's rule.
// Scales.  The accumulator rows of a lane are keys 4 g .. 4 g + 3 of a tile: it needs those keys' k_scale and v_scale.  Each lane loads
// ONE fp32 scale through the slot map (g = 0 / 1: k_scale of its key in tile A / B, g = 2 / 3: v_scale likewise), the wave passes them
// through 256 bytes of its own LDS and every lane reads its four rows of each as 16-byte pieces.
// Softmax.  Online (m, l) per head and wave: a lane's 8 logits, then the four lane groups (two shuffles).
// P.V.  O^T[D x 16] += V^T . P^T, 16x16x32 over the 32 keys of a step.  The accumulator layout of the two S^T tiles IS the B operand
// layout (slot e < 4: key 4 g + e of tile A, else key 4 g + e - 4 of tile B); V^T is read from LDS with ds_read_b64_tr_b16 in the same key
// order.  v_scale[row] varies along the keys, the MFMA's k-dimension, so it enters BEFORE the MFMA — folded into P in fp32, p' = p *
// v_scale, as the VALU stream folds it — and the V codes are widened to bf16 with scale 1 (exact).  p' is a bf16 pair hi + lo (16
// significant bits); the PV MFMA is the bf16 one in BOTH element-type builds: p * v_scale has no bound fp16 could hold (a row holding
// 60000 has scale 134, a tiny row 2^-27), bf16 keeps fp32's exponent range.  l sums the unscaled p.
// Load policy.  Every K and V byte is read exactly once by one lane: non-temporal loads, as every stream of this library reads rows it
// will not touch again in the launch.  The bank's resident_bytes policy does not apply (a quantised plan has no resident rows).
// Appended row.  The workgroup whose range holds position T - 1 quantises k_new / v_new by the rule of ekv_kv8_quantize with the FP8
// stream's own helpers (ekv_widen8_amax, ekv_group_max, ekv_fp8_row_scale, ekv_fp8_quant4: the same bits) — wave 0, D / 16 lanes with 16
// elements each — stores codes and scales, and attends the row AS QUANTISED as a one-key tile through the same code (the codes travel
// through LDS into the operand layout).
// Outputs.  The waves' (m, l, o) are exchanged through LDS (each wave's slice lives in its own V tile) and combined; partial stores are
// sc1 stores when the launch folds; the last-arriver fold is the protocol of ekv_attn_decode.inc (no spin-wait).  A range without a live
// row stores (-inf, 0, 0) and still arrives.  Every store is a vector store.
#include "ekv_common.h"
#include "ekv_kernels.h"

#if EKV_BF16
#define ekv_attn_decode_g8_kernel ekv_attn_decode_g8_kernel_bf16
#endif

namespace {

typedef float g8_f4 __attribute__((ext_vector_type(4)));
typedef __bf16 g8_b2 __attribute__((ext_vector_type(2)));
typedef __bf16 g8_b4 __attribute__((ext_vector_type(4)));
typedef __bf16 g8_b8 __attribute__((ext_vector_type(8)));
typedef short g8_s4 __attribute__((ext_vector_type(4)));

constexpr int kG8D = EKV_D;
static_assert(kG8D == 64 || kG8D == 128, "FP8 rows: head_dim 64 / 128");
constexpr int kG8KT = kDecodeG8KT;            // keys per wave step: two 16-key MFMA tiles
constexpr int kG8NK = kG8D / 32;              // logit MFMAs per tile
constexpr int kG8NW = kG8D / 16;              // 4-byte words of a lane's D / 4 contiguous codes of a row; also the 16-column blocks of O^T
constexpr int kG8RS = kG8D + kChunkPadH;      // V tile row stride in bf16 elements
constexpr int kG8XS = 2 + kG8D / 4 + 1;       // floats per lane of the wave exchange: (m, l, o[D / 16][4]) + 1 (odd pitch)
constexpr size_t kG8VTile = ekv_decode_g8_vtile(kG8D);      // bytes of a wave's V tile (ekv_geometry.h: the kernel's LDS plan and its row bound)
static_assert(kG8VTile == (size_t)kG8KT * kG8RS * 2, "the V tile of the LDS plan");
static_assert((size_t)64 * kG8XS * 4 <= kG8VTile, "a wave's exchange slice fits its V tile");

struct G8Tile {      // a wave step in flight: this lane's D / 4 K and V codes of its key in tile A / B, and its one scale
  uint32_t kA[kG8NW], kB[kG8NW], vA[kG8NW], vB[kG8NW];
  float sc;
};

// LDS traffic of ONE wave: orders its own writes and reads (the hardware runs a wave's LDS operations in order)
__device__ __forceinline__ void g8_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// the 8 codes of two words, widened to the element type with scale 1 (exact)
__device__ __forceinline__ ekv_h8 g8_widen_e(uint32_t w0, uint32_t w1) {
  const ekv_h2 a = ekv_fp8_pk_e<false>(w0), b = ekv_fp8_pk_e<true>(w0), c = ekv_fp8_pk_e<false>(w1), d = ekv_fp8_pk_e<true>(w1);
  return ekv_h8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
// ... to bf16 (exact: 3 mantissa bits)
__device__ __forceinline__ g8_b8 g8_widen_b(uint32_t w0, uint32_t w1) {
  const g8_b2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true);
  const g8_b2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true);
  return g8_b8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
// D / 4 contiguous bytes of a code row, in 16-byte non-temporal loads
__device__ __forceinline__ void g8_load_codes(const char* p, uint32_t (&w)[kG8NW]) {
#pragma unroll
  for (int i = 0; i < kG8NW / 4; ++i) {
    const ekv_u4 x = __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(p) + i);
    w[4 * i] = x[0], w[4 * i + 1] = x[1], w[4 * i + 2] = x[2], w[4 * i + 3] = x[3];
  }
}

__global__ void __launch_bounds__(256) ekv_attn_decode_g8_kernel(const EkvAttnArgs a) {
  constexpr int D = kG8D, RS = kG8RS, NK = kG8NK, NW = kG8NW, PS = EkvDecodeGeom<kG8D>::PS;
  constexpr int LPR = D / 16;      // lanes that quantise the appended row: 16 elements each (the FP8 stream's lane group)
  constexpr float kMFloor = -1.0e30f;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int split = blockIdx.x, h = blockIdx.y, ll = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int rep = a.n_q_heads / a.n_kv_heads, hq0 = h * rep;
  const int t0 = split * a.rows_per_split, t_end = min(a.n_slots, t0 + a.rows_per_split);
  const int t_new = a.n_slots - 1;      // the appended position
  const bool has_new = t_new >= t0 && t_new < t_end;
  const int t1 = has_new ? t_new : t_end;      // the stream covers [t0, t1); the appended row follows from k_new / v_new
  const size_t head_row = ((size_t)(a.layer_begin + ll) * a.n_kv_heads + h) * a.cap;

  // LDS: slot entries of the range | per wave: V tile (bf16) | per wave: 4 x 16 scales | the appended row's K codes, V codes
  int32_t* s_slot = reinterpret_cast<int32_t*>(smem);
  char* const tiles = smem + ekv_align((size_t)a.rows_per_split * 4, 16);
  __bf16* sV = reinterpret_cast<__bf16*>(tiles + (size_t)wave * kG8VTile);
  float* sx = reinterpret_cast<float*>(tiles + 4 * kG8VTile) + wave * 64;
  uint32_t* s_new = reinterpret_cast<uint32_t*>(tiles + 4 * kG8VTile) + 4 * 64;      // K codes [32 words] | V codes [32 words]
  for (int i = tid; i < t_end - t0; i += 256) s_slot[i] = a.slot_of_pos[head_row + t0 + i];
  __syncthreads();

  // Q, the B operand of every logit MFMA: head c (zeros for a padded column), elements g * D / 4 + 8 i .. + 7
  const bool head_ok = c < rep;
  ekv_h8 qreg[NK];
#pragma unroll
  for (int i = 0; i < NK; ++i) {
    qreg[i] = ekv_h8{0, 0, 0, 0, 0, 0, 0, 0};
    if (head_ok) qreg[i] = __builtin_bit_cast(ekv_h8, reinterpret_cast<const uint4*>(a.q + ((size_t)ll * a.n_q_heads + hq0 + c) * D)[g * NK + i]);
  }
  float* const logit_row = a.logits ? a.logits + ((size_t)ll * a.n_q_heads + hq0 + c) * a.t_pad : nullptr;

  const char* const k_codes = reinterpret_cast<const char*>(a.k) + head_row * D;
  const char* const v_codes = reinterpret_cast<const char*>(a.v) + head_row * D;
  const float* const k_scales = a.k_scale + head_row;
  const float* const v_scales = a.v_scale + head_row;

  float m_run = EKV_NEG_INF, l_run = 0.f;      // of head c, over this lane's keys (l) / this wave's keys (m)
  g8_f4 oacc[NW];                              // O^T: d = 16 db + 4 g + e, head c
#pragma unroll
  for (int db = 0; db < NW; ++db) oacc[db] = g8_f4{0.f, 0.f, 0.f, 0.f};

  // rows of tile positions [j0, j0 + 32), clamped into the range (a clamped row is a live row: finite, and masked by its position)
  auto load = [&](int j0, G8Tile& t) {
    const int sA = s_slot[min(j0 + c, t1 - 1) - t0], sB = s_slot[min(j0 + 16 + c, t1 - 1) - t0];
    g8_load_codes(k_codes + (size_t)sA * D + g * (D / 4), t.kA);
    g8_load_codes(k_codes + (size_t)sB * D + g * (D / 4), t.kB);
    g8_load_codes(v_codes + (size_t)sA * D + g * (D / 4), t.vA);
    g8_load_codes(v_codes + (size_t)sB * D + g * (D / 4), t.vB);
    t.sc = ((g & 2) ? v_scales : k_scales)[(g & 1) ? sB : sA];
  };

  // one wave step: the keys at positions jbase + [0, 32) that lie below jlim
  auto process = [&](const G8Tile& t, int jbase, int jlim) {
    g8_wave_sync();      // (the previous step's reads of sx / sV are done)
    sx[g * 16 + c] = t.sc;
    // ---- V: codes g * D / 4 .. of key c (tile A) and of key 16 + c (tile B), widened, to the wave's tile
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      *reinterpret_cast<g8_b8*>(sV + c * RS + g * (D / 4) + i * 8) = g8_widen_b(t.vA[2 * i], t.vA[2 * i + 1]);
      *reinterpret_cast<g8_b8*>(sV + (16 + c) * RS + g * (D / 4) + i * 8) = g8_widen_b(t.vB[2 * i], t.vB[2 * i + 1]);
    }
    // ---- S^T = K . Q^T: one accumulator per tile (the row scale is constant along k)
    g8_f4 SA = {0.f, 0.f, 0.f, 0.f}, SB = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      SA = EKV_MFMA_16x16x32(g8_widen_e(t.kA[2 * i], t.kA[2 * i + 1]), qreg[i], SA, 0, 0, 0);
      SB = EKV_MFMA_16x16x32(g8_widen_e(t.kB[2 * i], t.kB[2 * i + 1]), qreg[i], SB, 0, 0, 0);
    }
    g8_wave_sync();      // (the scales and the V tile are written)
    // scales of this lane's accumulator rows (keys 4 g .. 4 g + 3 of tile A / B)
    const g8_f4 ksA = *reinterpret_cast<const g8_f4*>(sx + 4 * g), ksB = *reinterpret_cast<const g8_f4*>(sx + 16 + 4 * g);
    const g8_f4 vsA = *reinterpret_cast<const g8_f4*>(sx + 32 + 4 * g), vsB = *reinterpret_cast<const g8_f4*>(sx + 48 + 4 * g);
    float sv[8], vs[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sv[e] = EKV_LOGIT(SA[e] * ksA[e], a);
      sv[4 + e] = EKV_LOGIT(SB[e] * ksB[e], a);
      vs[e] = vsA[e], vs[4 + e] = vsB[e];
    }
    float mx = EKV_NEG_INF;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = jbase + (e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4));
      if (j >= jlim) sv[e] = EKV_NEG_INF;
      else if (logit_row != nullptr && head_ok) logit_row[j] = sv[e];
      mx = fmaxf(mx, sv[e]);
    }
    // ---- online softmax of head c; its four lane groups share the running maximum
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(fmaxf(m_run, mx), kMFloor);
    const float alpha = exp2f((m_run - mn) * EKV_LOG2E);
    g8_b8 bP = {0, 0, 0, 0, 0, 0, 0, 0}, bPl = {0, 0, 0, 0, 0, 0, 0, 0};
    float ls = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float p = exp2f((sv[e] - mn) * EKV_LOG2E);
      ls += p;
      const float pv = p * vs[e];      // (the row's V scale, folded into p in fp32)
      bP[e] = (__bf16)pv;
      bPl[e] = (__bf16)(pv - (float)bP[e]);
    }
    l_run = l_run * alpha + ls;
    m_run = mn;
#pragma unroll
    for (int db = 0; db < NW; ++db) oacc[db] = oacc[db] * alpha;
    // ---- O^T += V^T . P^T: lane c of group g receives column 16 db + c of rows 4 g .. 4 g + 3 of each 16-key tile
#pragma unroll
    for (int db = 0; db < NW; ++db) {
      const __bf16* vp = sV + (4 * g + (c >> 2)) * RS + db * 16 + 4 * (c & 3);
      const g8_b4 v_lo = __builtin_bit_cast(g8_b4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) g8_s4*)vp));
      const g8_b4 v_hi = __builtin_bit_cast(g8_b4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) g8_s4*)(vp + 16 * RS)));
      const g8_b8 aV = {v_lo[0], v_lo[1], v_lo[2], v_lo[3], v_hi[0], v_hi[1], v_hi[2], v_hi[3]};
      oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aV, bP, oacc[db], 0, 0, 0);
      oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aV, bPl, oacc[db], 0, 0, 0);
    }
  };

  // ---- the stream: wave w takes tiles w, w + 4, ... of the range, the next tile's loads in flight under the current one
  {
    const int n_tiles = t1 > t0 ? (t1 - t0 + kG8KT - 1) / kG8KT : 0;
    G8Tile cur = {}, nxt = {};
    if (wave < n_tiles) load(t0 + wave * kG8KT, cur);
    for (int it = wave; it < n_tiles; it += 4) {
      if (it + 4 < n_tiles) load(t0 + (it + 4) * kG8KT, nxt);
      process(cur, t0 + it * kG8KT, t1);
      cur = nxt;
    }
  }

  // ---- the appended row: quantised by wave 0 (every lane group of LPR lanes computes the row, group 0 stores it), stored once, attended
  // as quantised as a one-key tile
  if (has_new && wave == 0) {
    const size_t row = head_row + s_slot[t_new - t0];
    const int sub = lane & (LPR - 1);
    float kf[16], vf[16];
    const uint4* kq = reinterpret_cast<const uint4*>(a.k_new + ((size_t)ll * a.n_kv_heads + h) * D) + sub * 2;
    const uint4* vq = reinterpret_cast<const uint4*>(a.v_new + ((size_t)ll * a.n_kv_heads + h) * D) + sub * 2;
    const float ka = fmaxf(ekv_widen8_amax(kq[0], kf), ekv_widen8_amax(kq[1], kf + 8));
    const float va = fmaxf(ekv_widen8_amax(vq[0], vf), ekv_widen8_amax(vq[1], vf + 8));
    const float ksn = ekv_fp8_row_scale(ekv_group_max<LPR>(ka)), vsn = ekv_fp8_row_scale(ekv_group_max<LPR>(va));
    const uint4 kn = uint4{ekv_fp8_quant4(kf[0], kf[1], kf[2], kf[3], ksn), ekv_fp8_quant4(kf[4], kf[5], kf[6], kf[7], ksn),
                           ekv_fp8_quant4(kf[8], kf[9], kf[10], kf[11], ksn), ekv_fp8_quant4(kf[12], kf[13], kf[14], kf[15], ksn)};
    const uint4 vn = uint4{ekv_fp8_quant4(vf[0], vf[1], vf[2], vf[3], vsn), ekv_fp8_quant4(vf[4], vf[5], vf[6], vf[7], vsn),
                           ekv_fp8_quant4(vf[8], vf[9], vf[10], vf[11], vsn), ekv_fp8_quant4(vf[12], vf[13], vf[14], vf[15], vsn)};
    if (lane < LPR) {
      reinterpret_cast<uint4*>(reinterpret_cast<char*>(a.k_w) + row * D)[sub] = kn;
      reinterpret_cast<uint4*>(reinterpret_cast<char*>(a.v_w) + row * D)[sub] = vn;
      *reinterpret_cast<uint4*>(s_new + 4 * sub) = kn;
      *reinterpret_cast<uint4*>(s_new + 32 + 4 * sub) = vn;
      if (sub == 0) {
        a.k_scale[row] = ksn;
        a.v_scale[row] = vsn;
      }
    }
    g8_wave_sync();
    G8Tile t = {};      // (zero codes under scale 1 everywhere but key 0 of tile A)
    t.sc = 1.f;
    if (c == 0) {
#pragma unroll
      for (int w = 0; w < NW; ++w) t.kA[w] = s_new[g * NW + w], t.vA[w] = s_new[32 + g * NW + w];
      if (g == 0) t.sc = ksn;
      if (g == 2) t.sc = vsn;
    }
    process(t, t_new, t_new + 1);
  }

  // ---- the waves' (m, l, o) through LDS (each wave's slice in its own V tile), combined per (head, d)
  if (m_run <= kMFloor) m_run = EKV_NEG_INF;      // -inf = "no key seen"
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  g8_wave_sync();
  {
    float* mine = reinterpret_cast<float*>(sV) + lane * kG8XS;
    mine[0] = m_run;
    mine[1] = l_run;
#pragma unroll
    for (int db = 0; db < NW; ++db)
#pragma unroll
      for (int e = 0; e < 4; ++e) mine[2 + db * 4 + e] = oacc[db][e];
  }
  __syncthreads();
  const bool fold_here = a.arrive != nullptr;
  for (int idx = tid; idx < rep * D; idx += 256) {
    const int r = idx / D, d = idx % D;
    const int src = (((d & 15) >> 2) * 16 + r) * kG8XS, eo = 2 + (d >> 4) * 4 + (d & 3);      // lane (g = d % 16 / 4, c = r), slot (db, e)
    float mw[4], mm = EKV_NEG_INF;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      mw[w] = reinterpret_cast<const float*>(tiles + (size_t)w * kG8VTile)[src];
      mm = fmaxf(mm, mw[w]);
    }
    float ls = 0.f, os = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float* p = reinterpret_cast<const float*>(tiles + (size_t)w * kG8VTile) + src;
      const float wt = mw[w] == EKV_NEG_INF ? 0.f : exp2f((mw[w] - mm) * EKV_LOG2E);
      ls += p[1] * wt;
      os += p[eo] * wt;
    }
    float* dst = a.partials + (((size_t)ll * a.n_q_heads + hq0 + r) * a.n_split + split) * PS;
    if (fold_here) {      // partials another workgroup of this launch will read: write-through stores
      if (d == 0) {
        ekv_store_sc1(dst, mm);
        ekv_store_sc1(dst + 1, ls);
      }
      ekv_store_sc1(dst + 2 + d, os);
    } else {
      if (d == 0) {
        dst[0] = mm;
        dst[1] = ls;
      }
      dst[2 + d] = os;
    }
  }
  if (!fold_here) return;
  // ---- in-kernel fold by the last split of the head to arrive: the protocol of ekv_attn_decode_kernel (ekv_attn_decode.inc, "in-kernel
  // fold"), step for step.  THE SAME SEQUENCE STANDS THERE and in ekv_attn_decode_mxg.inc: a change to one site goes to all three (a shared
  // helper would have to leave those files' objects byte-identical; until a change that re-records them, the sites point at each other) —
  // sc1 partial stores, every wave drains its stores, barrier, ONE agent-scope fetch_add on the head's arrival counter (the last arriver
  // leaves it at zero), sc1 buffer loads of the partials.  No spin-wait.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  uint32_t* s_last = reinterpret_cast<uint32_t*>(tiles);      // (the exchange slices have been consumed)
  if (tid == 0) {
    uint32_t* word = a.arrive + (size_t)ll * a.n_kv_heads + h;
    const uint32_t old = __hip_atomic_fetch_add(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = (int)(old + 1u) == a.n_split;
    if (last) __hip_atomic_store(word, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = last ? 1u : 0u;
  }
  __syncthreads();
  if (*s_last == 0u) return;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      a.partials + (size_t)ll * a.n_q_heads * a.n_split * PS, 0, (int)((size_t)a.n_q_heads * a.n_split * PS * 4), 0x00020000);
  for (int idx = tid; idx < rep * D; idx += 256) {
    const int r = idx / D, d = idx % D;
    a.out_direct[((size_t)ll * a.n_q_heads + hq0 + r) * D + d] = ekv_to_e(ekv_fold_partials_buf_auto(rsrc, (unsigned)((hq0 + r) * a.n_split * PS), a.n_split, PS, d));
  }
}

}  // namespace

hipError_t EKV_FN_D_ELEM(ekv_launch_attn_decode_g8, EKV_D, EKV_ELEM)(const EkvAttnArgs& a, int layer_count, hipStream_t s) {
  const int rep = a.n_q_heads / a.n_kv_heads;
  if (rep < 1 || rep > 16 || a.k_scale == nullptr || a.v_scale == nullptr || a.rows_per_split < 1 || a.rows_per_split > ekv_decode_g8_max_rows(EKV_D))
    return hipErrorInvalidValue;      // (the planner never sends a longer range)
  const size_t lds = ekv_decode_g8_lds(EKV_D, a.rows_per_split);
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_attn_decode_g8_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(ekv_attn_decode_g8_kernel, dim3(a.n_split, a.n_kv_heads, layer_count), dim3(256), lds, s, a);
  return hipGetLastError();
}
