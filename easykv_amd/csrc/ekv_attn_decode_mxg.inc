// ekv_attn_decode_mxg_kernel: the split-path decode kernel for MXFP4 rows at GQA factors up to 16 ("kv4 gqa", include/easykv_hip.h; the
// ekv_kv4_gqa_* calls), MFMA 16x16x32.  head_dim 128, plain keys; compiled once per element type by the EKV_DECODE_MXG lines of the
// manifest, launch code in ekv_attn_decode_mxg.hip.  It keeps the contract of ekv_attn_decode_kernel (ekv_attn_decode.inc): fp32 logits to
// a.logits, (m, l, o[D]) partials per query head and split to a.partials, the appended row quantised and stored once, the optional
// last-arriver fold over a.arrive — so the fold, both scorers and the range compaction behind it are the 16-bit instances.
//
// Why it exists.  The VALU stream gives each lane one 32-element block of a row and a 32-float output slice PER QUERY HEAD: registers grow
// linearly with the GQA factor (no REP = 8 build, REP = 2 / 4 spill).  Here the query heads of a KV head are the 16 columns of one MFMA
// tile: 16 heads cost what one costs, and a wave's whole 128 x 16 output is 32 accumulator registers.
//
// Work split.  One workgroup of 4 waves per (key-range split, KV head, layer); there is no query-head-group factor: all rep <= 16 query
// heads share ONE stream of the head's K/V.  The slot entries of the range are staged in LDS once.  Wave w takes the 32-key tiles w,
// w + 4, ... of the range and runs them on its own, without a workgroup barrier: it has its own V tile, exponent words and online
// (m, l, o) state; the loads of its next tile fly while it consumes the current one.  Lane (g = lane / 16, c = lane % 16).
//
// Logits.  S^T[16 keys x 16 heads] per 16-key tile, two tiles (A: keys 0..15, B: 16..31) per step.  Q is the B operand, loaded once:
// lane (g, c) holds elements 32 kb + 8 g .. + 7 of head c for kb = 0..3, zeros for c >= rep (padded columns are never stored).  K is the A
// operand straight from global memory: lane (g, c) loads word g of block kb of key c (4 bytes = 8 codes) and widens it to the element
// type with scale 1 (v_cvt_scalef32_pk_{f16,bf16}_fp4: exact).  One MFMA's k-extent is one scale block, so block kb runs into a zeroed
// accumulator and the logit is sum_b 2^e(key, b) * acc_b in fp32, b = 0..3 in that order, then / sm_div — the VALU stream's rule.  The
// accumulator rows of a lane are keys 4 g .. 4 g + 3 of a tile: it needs those keys' exponent words.  Each lane loads ONE exponent word
// (g = 0 / 1: K of its key in tile A / B, g = 2 / 3: V likewise), the wave passes them through 256 bytes of LDS and every lane reads the
// four rows it needs as 16-byte pieces.
// Softmax.  Online (m, l) per head and wave: a lane's 8 logits, then the four lane groups (two shuffles).
// P.V.  O^T[128 x 16] += V^T . P^T, 16x16x32 over the 32 keys of a step.  The accumulator layout of the two S^T tiles IS the B operand
// layout (slot e < 4: key 4 g + e of tile A, else key 4 g + e - 4 of tile B); V^T is read from LDS with ds_read_b64_tr_b16 in the same key
// order.  V's block scale varies along the keys, the MFMA's k-dimension, so it is applied BEFORE the MFMA: the codes are widened to bf16
// WITH the block's scale (v_cvt_scalef32_pk_bf16_fp4: code * 2^e has one mantissa bit and bf16 has fp32's exponent range, so this is exact
// for every exponent byte, 14 included, where fp16 would overflow at 6 * 2^14) and P is a bf16 pair hi + lo (16 significant bits: the
// MFMA pipe has the room, the kernel streams memory).  The PV MFMA is the bf16 one in both element-type builds.  Candidates and their
// errors: DESIGN.md §3.24 / §8.
// Load policy.  A V block is read exactly once, by one 16-byte load: non-temporal, as every stream of this library reads rows it will not
// touch again in the launch.  A K row is read by four 4-byte loads per lane group (one per scale block), which hit the same 64-byte row
// back to back: default policy, so the row's line stays in the cache between them.  The bank's resident_bytes policy does not apply:
// resident rows belong to the 16-bit one-launch instances, and every quantised plan has none (resolve_call clears fused_order).
// Appended row.  The workgroup whose range holds position T - 1 quantises k_new / v_new by the rule of ekv_kv4_quantize (ekv_fp4_quant_block,
// the VALU stream's helper: the same bits), four lanes of wave 0, one block each; stores codes and exponent bytes; and attends the row AS
// QUANTISED as a one-key tile through the same code (the codes travel through LDS into the operand layout).
// Outputs.  The waves' (m, l, o) are exchanged through LDS (each wave's slice lives in its own V tile) and combined; partial stores are
// sc1 stores when the launch folds; the last-arriver fold is the protocol of ekv_attn_decode.inc (no spin-wait).  A range without a live
// row stores (-inf, 0, 0) and still arrives.  No scalar memory writes; every store is a vector store.
#include "ekv_common.h"
#include "ekv_kernels.h"

#if EKV_BF16
#define ekv_attn_decode_mxg_kernel ekv_attn_decode_mxg_kernel_bf16
#endif

namespace {

typedef float mxg_f4 __attribute__((ext_vector_type(4)));
typedef __bf16 mxg_b2 __attribute__((ext_vector_type(2)));
typedef __bf16 mxg_b4 __attribute__((ext_vector_type(4)));
typedef __bf16 mxg_b8 __attribute__((ext_vector_type(8)));
typedef short mxg_s4 __attribute__((ext_vector_type(4)));

constexpr int kMxgD = 128;
constexpr int kMxgKT = kDecodeMxgKT;           // keys per wave step: two 16-key MFMA tiles
constexpr int kMxgRS = kMxgD + kChunkPadH;    // V tile row stride in bf16 elements (conflict-free transposing reads of 4 rows x 32 B)
constexpr int kMxgXS = 35;                    // floats per lane of the wave exchange: (m, l, o[8][4]) + 1 (odd pitch)
constexpr size_t kMxgVTile = kDecodeMxgVTile;      // bytes of a wave's V tile (ekv_geometry.h: the kernel's LDS plan and its row bound)
static_assert(kMxgVTile == (size_t)kMxgKT * kMxgRS * 2, "the V tile of the LDS plan");
static_assert((size_t)64 * kMxgXS * 4 <= kMxgVTile, "a wave's exchange slice fits its V tile");

struct MxgTile {      // a wave step in flight: this lane's K words (block kb, word g of its key in tile A / B), V blocks and exponent word
  uint32_t kA[4], kB[4];
  uint4 vA, vB;
  uint32_t ex;
};

// LDS traffic of ONE wave: orders its own writes and reads (the hardware runs a wave's LDS operations in order)
__device__ __forceinline__ void mxg_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// the 8 codes of one word, widened to the element type with scale 1 (exact)
__device__ __forceinline__ ekv_h8 mxg_widen_e(uint32_t w) {
  const ekv_h2 a = ekv_fp4_pk_e<0>(w), b = ekv_fp4_pk_e<1>(w), c = ekv_fp4_pk_e<2>(w), d = ekv_fp4_pk_e<3>(w);
  return ekv_h8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
// the 8 codes of one word times the block's scale, as bf16 (exact: one mantissa bit, fp32's exponent range)
__device__ __forceinline__ mxg_b8 mxg_widen_scaled(uint32_t w, float scale) {
  const mxg_b2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1);
  const mxg_b2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3);
  return mxg_b8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
// sum_b 2^e_b * s_b, b = 0..3 in order: the block scales applied to the blocks' partial dot products in fp32
__device__ __forceinline__ float mxg_combine(uint32_t ew, float s0, float s1, float s2, float s3) {
  float acc = s0 * ekv_fp4_exp_scale(ew & 0xFFu);
  acc += s1 * ekv_fp4_exp_scale((ew >> 8) & 0xFFu);
  acc += s2 * ekv_fp4_exp_scale((ew >> 16) & 0xFFu);
  acc += s3 * ekv_fp4_exp_scale(ew >> 24);
  return acc;
}

__global__ void __launch_bounds__(256) ekv_attn_decode_mxg_kernel(const EkvAttnArgs a) {
  constexpr int D = kMxgD, RS = kMxgRS, PS = EkvDecodeGeom<kMxgD>::PS;
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

  // LDS: slot entries of the range | per wave: V tile (bf16, scaled) | per wave: 4 x 16 exponent words | the appended row's codes
  int32_t* s_slot = reinterpret_cast<int32_t*>(smem);
  char* const tiles = smem + ekv_align((size_t)a.rows_per_split * 4, 16);
  __bf16* sV = reinterpret_cast<__bf16*>(tiles + (size_t)wave * kMxgVTile);
  uint32_t* sx = reinterpret_cast<uint32_t*>(tiles + 4 * kMxgVTile) + wave * 64;
  uint32_t* s_new = reinterpret_cast<uint32_t*>(tiles + 4 * kMxgVTile) + 4 * 64;      // K codes [16] | V codes [16] | K, V exponent words
  for (int i = tid; i < t_end - t0; i += 256) s_slot[i] = a.slot_of_pos[head_row + t0 + i];
  __syncthreads();

  // Q, the B operand of every logit MFMA: head c (zeros for a padded column), elements 32 kb + 8 g .. + 7
  const bool head_ok = c < rep;
  ekv_h8 qreg[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    qreg[kb] = ekv_h8{0, 0, 0, 0, 0, 0, 0, 0};
    if (head_ok) qreg[kb] = __builtin_bit_cast(ekv_h8, reinterpret_cast<const uint4*>(a.q + ((size_t)ll * a.n_q_heads + hq0 + c) * D + kb * 32)[g]);
  }
  float* const logit_row = a.logits ? a.logits + ((size_t)ll * a.n_q_heads + hq0 + c) * a.t_pad : nullptr;

  const char* const k_codes = reinterpret_cast<const char*>(a.k) + head_row * (D / 2);
  const char* const v_codes = reinterpret_cast<const char*>(a.v) + head_row * (D / 2);
  const uint32_t* const k_exps = reinterpret_cast<const uint32_t*>(a.k_exp + head_row * 4);
  const uint32_t* const v_exps = reinterpret_cast<const uint32_t*>(a.v_exp + head_row * 4);

  float m_run = EKV_NEG_INF, l_run = 0.f;      // of head c, over this lane's keys (l) / this wave's keys (m)
  mxg_f4 oacc[8];                              // O^T: d = 16 db + 4 g + e, head c
#pragma unroll
  for (int db = 0; db < 8; ++db) oacc[db] = mxg_f4{0.f, 0.f, 0.f, 0.f};

  // rows of tile positions [j0, j0 + 32), clamped into the range (a clamped row is a live row: finite, and masked by its position)
  auto load = [&](int j0, MxgTile& t) {
    const int sA = s_slot[min(j0 + c, t1 - 1) - t0], sB = s_slot[min(j0 + 16 + c, t1 - 1) - t0];
    const char* const pA = k_codes + (size_t)sA * (D / 2) + g * 4;
    const char* const pB = k_codes + (size_t)sB * (D / 2) + g * 4;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      t.kA[kb] = *reinterpret_cast<const uint32_t*>(pA + kb * 16);
      t.kB[kb] = *reinterpret_cast<const uint32_t*>(pB + kb * 16);
    }
    t.vA = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(v_codes + (size_t)sA * (D / 2)) + g));
    t.vB = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(v_codes + (size_t)sB * (D / 2)) + g));
    t.ex = ((g & 2) ? v_exps : k_exps)[(g & 1) ? sB : sA];
  };

  // one wave step: the keys at positions jbase + [0, 32) that lie below jlim
  auto process = [&](const MxgTile& t, int jbase, int jlim) {
    mxg_wave_sync();      // (the previous step's reads of sx / sV are done)
    sx[g * 16 + c] = t.ex;
    mxg_wave_sync();
    // exponent words of this lane's accumulator rows (keys 4 g .. 4 g + 3 of tile A / B), and of the blocks it stages
    const uint4 keA = *reinterpret_cast<const uint4*>(sx + 4 * g), keB = *reinterpret_cast<const uint4*>(sx + 16 + 4 * g);
    const float vsA = ekv_fp4_exp_scale((sx[32 + c] >> (8 * g)) & 0xFFu), vsB = ekv_fp4_exp_scale((sx[48 + c] >> (8 * g)) & 0xFFu);
    // ---- V: block g of key c (tile A) and of key 16 + c (tile B), scaled and widened, to the wave's tile
    {
      const uint32_t wa[4] = {t.vA.x, t.vA.y, t.vA.z, t.vA.w}, wb[4] = {t.vB.x, t.vB.y, t.vB.z, t.vB.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<mxg_b8*>(sV + c * RS + g * 32 + i * 8) = mxg_widen_scaled(wa[i], vsA);
        *reinterpret_cast<mxg_b8*>(sV + (16 + c) * RS + g * 32 + i * 8) = mxg_widen_scaled(wb[i], vsB);
      }
    }
    // ---- S^T = K . Q^T, one zeroed accumulator per scale block
    mxg_f4 SA[4], SB[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      SA[kb] = EKV_MFMA_16x16x32(mxg_widen_e(t.kA[kb]), qreg[kb], (mxg_f4{0.f, 0.f, 0.f, 0.f}), 0, 0, 0);
      SB[kb] = EKV_MFMA_16x16x32(mxg_widen_e(t.kB[kb]), qreg[kb], (mxg_f4{0.f, 0.f, 0.f, 0.f}), 0, 0, 0);
    }
    const uint32_t ewA[4] = {keA.x, keA.y, keA.z, keA.w}, ewB[4] = {keB.x, keB.y, keB.z, keB.w};
    float sv[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sv[e] = EKV_LOGIT(mxg_combine(ewA[e], SA[0][e], SA[1][e], SA[2][e], SA[3][e]), a);
      sv[4 + e] = EKV_LOGIT(mxg_combine(ewB[e], SB[0][e], SB[1][e], SB[2][e], SB[3][e]), a);
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
    mxg_b8 bP = {0, 0, 0, 0, 0, 0, 0, 0}, bPl = {0, 0, 0, 0, 0, 0, 0, 0};
    float ls = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float p = exp2f((sv[e] - mn) * EKV_LOG2E);
      ls += p;
      bP[e] = (__bf16)p;
      bPl[e] = (__bf16)(p - (float)bP[e]);
    }
    l_run = l_run * alpha + ls;
    m_run = mn;
#pragma unroll
    for (int db = 0; db < 8; ++db) oacc[db] = oacc[db] * alpha;
    mxg_wave_sync();      // (the V tile is written)
    // ---- O^T += V^T . P^T: lane c of group g receives column 16 db + c of rows 4 g .. 4 g + 3 of each 16-key tile
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      const __bf16* vp = sV + (4 * g + (c >> 2)) * RS + db * 16 + 4 * (c & 3);
      const mxg_b4 v_lo = __builtin_bit_cast(mxg_b4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) mxg_s4*)vp));
      const mxg_b4 v_hi = __builtin_bit_cast(mxg_b4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) mxg_s4*)(vp + 16 * RS)));
      const mxg_b8 aV = {v_lo[0], v_lo[1], v_lo[2], v_lo[3], v_hi[0], v_hi[1], v_hi[2], v_hi[3]};
      oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aV, bP, oacc[db], 0, 0, 0);
      oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aV, bPl, oacc[db], 0, 0, 0);
    }
  };

  // ---- the stream: wave w takes tiles w, w + 4, ... of the range, the next tile's loads in flight under the current one
  {
    const int n_tiles = t1 > t0 ? (t1 - t0 + kMxgKT - 1) / kMxgKT : 0;
    MxgTile cur = {}, nxt = {};
    if (wave < n_tiles) load(t0 + wave * kMxgKT, cur);
    for (int it = wave; it < n_tiles; it += 4) {
      if (it + 4 < n_tiles) load(t0 + (it + 4) * kMxgKT, nxt);
      process(cur, t0 + it * kMxgKT, t1);
      cur = nxt;
    }
  }

  // ---- the appended row: quantised by four lanes (one block each), stored once, attended as quantised as a one-key tile
  if (has_new && wave == 0) {
    const size_t row = head_row + s_slot[t_new - t0];
    if (lane < 4) {
      uint32_t ke, ve;
      const uint4 kn = ekv_fp4_quant_block(reinterpret_cast<const uint4*>(a.k_new + ((size_t)ll * a.n_kv_heads + h) * D) + lane * 4, ke);
      const uint4 vn = ekv_fp4_quant_block(reinterpret_cast<const uint4*>(a.v_new + ((size_t)ll * a.n_kv_heads + h) * D) + lane * 4, ve);
      reinterpret_cast<uint4*>(reinterpret_cast<char*>(a.k_w) + row * (D / 2))[lane] = kn;
      reinterpret_cast<uint4*>(reinterpret_cast<char*>(a.v_w) + row * (D / 2))[lane] = vn;
      a.k_exp[row * 4 + lane] = (uint8_t)ke;
      a.v_exp[row * 4 + lane] = (uint8_t)ve;
      *reinterpret_cast<uint4*>(s_new + 4 * lane) = kn;
      *reinterpret_cast<uint4*>(s_new + 16 + 4 * lane) = vn;
      reinterpret_cast<uint8_t*>(s_new + 32)[lane] = (uint8_t)ke;
      reinterpret_cast<uint8_t*>(s_new + 33)[lane] = (uint8_t)ve;
    }
    mxg_wave_sync();
    MxgTile t = {};      // (zero codes under scale 1 everywhere but key 0 of tile A)
    t.ex = 0x7F7F7F7Fu;
    if (c == 0) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) t.kA[kb] = s_new[4 * kb + g];
      t.vA = *reinterpret_cast<const uint4*>(s_new + 16 + 4 * g);
      if (!(g & 1)) t.ex = s_new[32 + (g >> 1)];
    }
    process(t, t_new, t_new + 1);
  }

  // ---- the waves' (m, l, o) through LDS (each wave's slice in its own V tile), combined per (head, d)
  if (m_run <= kMFloor) m_run = EKV_NEG_INF;      // -inf = "no key seen"
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  mxg_wave_sync();
  {
    float* mine = reinterpret_cast<float*>(sV) + lane * kMxgXS;
    mine[0] = m_run;
    mine[1] = l_run;
#pragma unroll
    for (int db = 0; db < 8; ++db)
#pragma unroll
      for (int e = 0; e < 4; ++e) mine[2 + db * 4 + e] = oacc[db][e];
  }
  __syncthreads();
  const bool fold_here = a.arrive != nullptr;
  for (int idx = tid; idx < rep * D; idx += 256) {
    const int r = idx / D, d = idx % D;
    const int src = (((d & 15) >> 2) * 16 + r) * kMxgXS, eo = 2 + (d >> 4) * 4 + (d & 3);      // lane (g = d % 16 / 4, c = r), slot (db, e)
    float mw[4], mm = EKV_NEG_INF;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      mw[w] = reinterpret_cast<const float*>(tiles + (size_t)w * kMxgVTile)[src];
      mm = fmaxf(mm, mw[w]);
    }
    float ls = 0.f, os = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float* p = reinterpret_cast<const float*>(tiles + (size_t)w * kMxgVTile) + src;
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
  // fold"), step for step.  THE SAME SEQUENCE STANDS THERE: a change to either site goes to both (a shared helper would have to leave
  // that file's objects byte-identical; until a change that re-records them, the two sites point at each other) — sc1 partial stores, every wave drains its stores, barrier, ONE agent-scope fetch_add on the head's arrival
  // counter (the last arriver leaves it at zero), sc1 buffer loads of the partials.  No spin-wait.
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

hipError_t EKV_FN_D_ELEM(ekv_launch_attn_decode_mxg, 128, EKV_ELEM)(const EkvAttnArgs& a, int layer_count, hipStream_t s) {
  const int rep = a.n_q_heads / a.n_kv_heads;
  if (rep < 1 || rep > 16 || a.k_exp == nullptr || a.v_exp == nullptr || a.rows_per_split > kDecodeMxgMaxRows) return hipErrorInvalidValue;      // (the planner never sends a longer range)
  const size_t lds = ekv_decode_mxg_lds(a.rows_per_split);
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_attn_decode_mxg_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(ekv_attn_decode_mxg_kernel, dim3(a.n_split, a.n_kv_heads, layer_count), dim3(256), lds, s, a);
  return hipGetLastError();
}
