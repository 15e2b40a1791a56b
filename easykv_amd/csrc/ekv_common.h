// Shared device helpers for the easykv_amd HIP kernels (gfx950 only, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "ekv_geometry.h"      // (ekv_align and the families' LDS plans)

#define EKV_WAVE 64
#define EKV_LOG2E 1.4426950408889634f
#define EKV_NEG_INF (-__builtin_inff())

// Element type of the 16-bit tensors (K/V rows, queries, outputs).  Every kernel instance is compiled for one of them: fp16, or
// bf16 with EKV_BF16 = 1 (the bf16 lines of ekv_instances.def, whose kernel names carry the tag _bf16).  Only what reads or
// writes an element differs: the dot / MFMA builtins, the widening to f32 and the rounding of f32 to 16 bits.  The row pointers of
// EkvAttnArgs / EkvScoreArgs stay __half*: rows are moved as bytes, and every element access goes through the helpers below.
#ifndef EKV_BF16
#define EKV_BF16 0
#endif
#if EKV_BF16
typedef __bf16 ekv_e;
#define EKV_DT_TAG _bf16
#define EKV_ELEM bf16
#define EKV_MFMA_16x16x32 __builtin_amdgcn_mfma_f32_16x16x32_bf16
#define EKV_MFMA_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_bf16
#else
typedef _Float16 ekv_e;
#define EKV_DT_TAG
#define EKV_ELEM f16
#define EKV_MFMA_16x16x32 __builtin_amdgcn_mfma_f32_16x16x32_f16
#define EKV_MFMA_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_f16
#endif
typedef ekv_e ekv_h2 __attribute__((ext_vector_type(2)));
typedef ekv_e ekv_h8 __attribute__((ext_vector_type(8)));
typedef unsigned int ekv_u4 __attribute__((ext_vector_type(4)));
typedef float ekv_f2 __attribute__((ext_vector_type(2)));

template <int CTRL>
__device__ __forceinline__ float ekv_dpp(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}

// The value of lane ^ 16: the partner across the DPP row boundary, inside each half of the wave (ds_swizzle, bit mode: and 0x1F, xor 0x10
// — no address register, no LDS memory touched).
__device__ __forceinline__ float ekv_swap_x16(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, x), 0x401F));
}

// All-reduce (sum) over aligned groups of LPR consecutive lanes, LPR in {4,8,16,32}; every lane gets the total.
// quad_perm[1,0,3,2], quad_perm[2,3,0,1], row_half_mirror, row_mirror: one fused v_add_f32_dpp each; 32 lanes (head_dim 256: a row is
// half a wave) take one more step across the DPP row boundary.
template <int LPR>
__device__ __forceinline__ float ekv_group_sum(float x) {
  static_assert(LPR == 4 || LPR == 8 || LPR == 16 || LPR == 32, "lane groups of 4, 8, 16 or 32 lanes");
  x += ekv_dpp<0xB1>(x);
  x += ekv_dpp<0x4E>(x);
  if (LPR >= 8) x += ekv_dpp<0x141>(x);
  if (LPR >= 16) x += ekv_dpp<0x140>(x);
  if constexpr (LPR >= 32) x += ekv_swap_x16(x);
  return x;
}

#if EKV_BF16
#define EKV_FDOT2 __builtin_amdgcn_fdot2_f32_bf16
#else
#define EKV_FDOT2 __builtin_amdgcn_fdot2
#endif
__device__ __forceinline__ float ekv_dot8(const uint4& a, const uint4& b, float acc) {
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, a.x), __builtin_bit_cast(ekv_h2, b.x), acc, false);
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, a.y), __builtin_bit_cast(ekv_h2, b.y), acc, false);
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, a.z), __builtin_bit_cast(ekv_h2, b.z), acc, false);
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, a.w), __builtin_bit_cast(ekv_h2, b.w), acc, false);
  return acc;
}

__device__ __forceinline__ void ekv_axpy8(float p, const uint4& v, float (&o)[8]) {
  const ekv_h8 h = __builtin_bit_cast(ekv_h8, v);
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = fmaf(p, (float)h[i], o[i]);
}

// ---- FP8 K/V rows ("kv8", include/easykv_hip.h): OCP e4m3fn codes, one fp32 scale per row, value = code * scale ----
// A lane's 16-byte piece of a row is 16 codes.  Widening a code to f16 / bf16 / f32 is exact (3 mantissa bits, 2^-9 .. 448), so the
// K side runs on the packed-pair dot product of the 16-bit builds (v_cvt_scalef32_pk_{f16,bf16}_fp8 with scale 1) and the V side on
// v_cvt_pk_f32_fp8 + fma; the row scales are applied to the fp32 logit and to p.
#define EKV_FP8_MAX 448.f
template <bool HI>
__device__ __forceinline__ ekv_h2 ekv_fp8_pk_e(uint32_t w) {
#if EKV_BF16
  return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI);
#else
  return __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, HI);
#endif
}
// 16 query elements (q0: 0..7, q1: 8..15) . 16 codes
__device__ __forceinline__ float ekv_dot16_fp8(const uint4& q0, const uint4& q1, const uint4& c, float acc) {
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, q0.x), ekv_fp8_pk_e<false>(c.x), acc, false);
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, q0.y), ekv_fp8_pk_e<true>(c.x), acc, false);
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, q0.z), ekv_fp8_pk_e<false>(c.y), acc, false);
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, q0.w), ekv_fp8_pk_e<true>(c.y), acc, false);
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, q1.x), ekv_fp8_pk_e<false>(c.z), acc, false);
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, q1.y), ekv_fp8_pk_e<true>(c.z), acc, false);
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, q1.z), ekv_fp8_pk_e<false>(c.w), acc, false);
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, q1.w), ekv_fp8_pk_e<true>(c.w), acc, false);
  return acc;
}
__device__ __forceinline__ void ekv_fp8_widen4(uint32_t w, float* f) {
  const ekv_f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
  f[0] = lo[0], f[1] = lo[1], f[2] = hi[0], f[3] = hi[1];
}
// o[0..16) += p * codes   (p already carries the row's V scale)
__device__ __forceinline__ void ekv_axpy16_fp8(float p, const uint4& c, float (&o)[16]) {
  float f[16];
  ekv_fp8_widen4(c.x, f), ekv_fp8_widen4(c.y, f + 4), ekv_fp8_widen4(c.z, f + 8), ekv_fp8_widen4(c.w, f + 12);
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = fmaf(p, f[i], o[i]);
}
// The quantisation rule of a row (include/easykv_hip.h): s = amax / 448 (1 for an all-zero row), code = RNE(x / s).  The division is
// the correctly rounded fp32 one, so x / s is bit for bit what the rule's restatement in torch computes; |x / s| <= 448 * (1 + 2^-23)
// rounds to a finite code, nothing saturates.
__device__ __forceinline__ float ekv_fp8_row_scale(float amax) { return amax == 0.f ? 1.f : amax / EKV_FP8_MAX; }
__device__ __forceinline__ uint32_t ekv_fp8_quant4(float a, float b, float c, float d, float s) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a / s, b / s, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c / s, d / s, w, true);
  return (uint32_t)w;
}
// max over aligned groups of LPR consecutive lanes (the lane pattern of ekv_group_sum)
template <int LPR>
__device__ __forceinline__ float ekv_group_max(float x) {
  static_assert(LPR == 4 || LPR == 8 || LPR == 16 || LPR == 32, "lane groups of 4, 8, 16 or 32 lanes");
  x = fmaxf(x, ekv_dpp<0xB1>(x));
  x = fmaxf(x, ekv_dpp<0x4E>(x));
  if (LPR >= 8) x = fmaxf(x, ekv_dpp<0x141>(x));
  if (LPR >= 16) x = fmaxf(x, ekv_dpp<0x140>(x));
  if constexpr (LPR >= 32) x = fmaxf(x, ekv_swap_x16(x));
  return x;
}
// |x| of the 8 16-bit elements of a 16-byte piece, widened to f32
__device__ __forceinline__ float ekv_widen8_amax(const uint4& v, float* f) {
  const ekv_h8 h = __builtin_bit_cast(ekv_h8, v);
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    f[i] = (float)h[i];
    m = fmaxf(m, fabsf(f[i]));
  }
  return m;
}

// ---- MXFP4 K/V rows ("kv4", include/easykv_hip.h): e2m1 codes, two per byte, one E8M0 exponent per 32-element block ----
// A lane's 16-byte piece of a row is the 32 codes of ONE block.  Widening a code is exact in every target type (one mantissa bit), so
// the K side runs on the packed-pair dot product of the 16-bit builds (v_cvt_scalef32_pk_{f16,bf16}_fp4 with scale 1, the block's 2^e
// applied to the lane's partial sum) and the V side on v_cvt_scalef32_pk_f32_fp4 with the block's scale + fma.
// Exponent byte of a block from its maximum: the smallest e with amax <= 6 * 2^e = 1.5 * 2^(e + 2), i.e. the float's own exponent
// minus 2, plus one when its mantissa exceeds 1.5 (the carry of the addition below); clamped to [-126, 127], 0 for an all-zero block.
__device__ __forceinline__ uint32_t ekv_fp4_block_exp(float amax) {
  if (amax == 0.f) return 127u;
  const int b = (int)((__float_as_uint(amax) + 0x3FFFFFu) >> 23) - 2;
  return (uint32_t)min(max(b, 1), 254);
}
// 2^(byte - 127) as the fp32 the conversions read their scale from (byte in [1, 254]: a normal number)
__device__ __forceinline__ float ekv_fp4_exp_scale(uint32_t byte) { return __uint_as_float(byte << 23); }
// 8 values -> 8 codes (one 32-bit word): RNE(x / scale), element 2i in the low nibble of byte i
__device__ __forceinline__ uint32_t ekv_fp4_quant8(const float* f, float scale) {
  uint32_t w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0u, f[0], f[1], scale, 0);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, f[2], f[3], scale, 1);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, f[4], f[5], scale, 2);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, f[6], f[7], scale, 3);
  return w;
}
template <int SEL>
__device__ __forceinline__ ekv_h2 ekv_fp4_pk_e(uint32_t w) {
#if EKV_BF16
  return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, SEL);
#else
  return __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, SEL);
#endif
}
// 8 query elements . the 8 codes of one word
__device__ __forceinline__ float ekv_dot8_fp4(const uint4& q, uint32_t c, float acc) {
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, q.x), ekv_fp4_pk_e<0>(c), acc, false);
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, q.y), ekv_fp4_pk_e<1>(c), acc, false);
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, q.z), ekv_fp4_pk_e<2>(c), acc, false);
  acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, q.w), ekv_fp4_pk_e<3>(c), acc, false);
  return acc;
}
// 32 query elements . the 32 codes of a block (the block's scale is the caller's business)
__device__ __forceinline__ float ekv_dot32_fp4(const uint4 (&q)[4], const uint4& c, float acc) {
  acc = ekv_dot8_fp4(q[0], c.x, acc);
  acc = ekv_dot8_fp4(q[1], c.y, acc);
  acc = ekv_dot8_fp4(q[2], c.z, acc);
  return ekv_dot8_fp4(q[3], c.w, acc);
}
// the 8 codes of one word times the block's scale, as fp32 (exact)
__device__ __forceinline__ void ekv_fp4_widen8(uint32_t w, float scale, float* f) {
  const ekv_f2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 0), b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 1);
  const ekv_f2 c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 2), d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 3);
  f[0] = a[0], f[1] = a[1], f[2] = b[0], f[3] = b[1], f[4] = c[0], f[5] = c[1], f[6] = d[0], f[7] = d[1];
}
// o[0..32) += p * (codes * scale)
__device__ __forceinline__ void ekv_axpy32_fp4(float p, float scale, const uint4& c, float (&o)[32]) {
  const uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float f[8];
    ekv_fp4_widen8(w[i], scale, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[8 * i + j] = fmaf(p, f[j], o[8 * i + j]);
  }
}
// o[0..16) += p * (codes * scale): half a block, the 16 codes of two words (FP8-key / MXFP4-value rows, "kv84": a lane pair per block)
__device__ __forceinline__ void ekv_axpy16_fp4(float p, float scale, const uint2& c, float (&o)[16]) {
  const uint32_t w[2] = {c.x, c.y};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    float f[8];
    ekv_fp4_widen8(w[i], scale, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[8 * i + j] = fmaf(p, f[j], o[8 * i + j]);
  }
}
// o[0..8) += p * (codes * scale): a quarter of a block, the 8 codes of one word (16-bit-key / MXFP4-value rows, "kv164": a lane quad per block)
__device__ __forceinline__ void ekv_axpy8_fp4(float p, float scale, uint32_t c, float (&o)[8]) {
  float f[8];
  ekv_fp4_widen8(c, scale, f);
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = fmaf(p, f[j], o[j]);
}
// 32 source elements (four 16-byte pieces) -> their block: 16 bytes of codes, the exponent byte in `e`
__device__ __forceinline__ uint4 ekv_fp4_quant_block(const uint4* src, uint32_t& e) {
  float f[32];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) amax = fmaxf(amax, ekv_widen8_amax(src[i], f + 8 * i));
  e = ekv_fp4_block_exp(amax);
  const float s = ekv_fp4_exp_scale(e);
  return uint4{ekv_fp4_quant8(f, s), ekv_fp4_quant8(f + 8, s), ekv_fp4_quant8(f + 16, s), ekv_fp4_quant8(f + 24, s)};
}

// ---- MXFP6 K/V rows ("kv6", include/easykv_hip.h): e2m3 codes, 32 per 24-byte block, one E8M0 exponent per 32-element block ----
// A lane's piece of a row is the 24 bytes of ONE block, 8-byte aligned (byte 24 * sub of a 96-byte row): three 8-byte loads into six
// registers.  Widening a code is exact in every target type (four significant bits), so the K side converts the block to 32 packed
// f16 / bf16 with scale 1 (v_cvt_scalef32_pk32_{f16,bf16}_fp6) and runs the packed-pair dot product of the 16-bit builds, the block's
// 2^e applied to the lane's partial sum; the V side converts with the block's scale (v_cvt_scalef32_pk32_f32_fp6) + fma.  The
// exponent plane and the fp32 form of a scale are kv4's (ekv_fp4_exp_scale).
typedef unsigned int ekv_u2 __attribute__((ext_vector_type(2)));
typedef unsigned int ekv_u6 __attribute__((ext_vector_type(6)));
typedef float ekv_f16x __attribute__((ext_vector_type(16)));
typedef float ekv_f32x __attribute__((ext_vector_type(32)));
typedef ekv_e ekv_h32 __attribute__((ext_vector_type(32)));
// Exponent byte of a block from its maximum: the smallest e with amax <= 7.5 * 2^e = 1.875 * 2^(e + 2), i.e. the float's own exponent
// minus 2, plus one when its mantissa exceeds 1.875 (the carry of the addition below); clamped to [-126, 127], 0 for an all-zero block.
__device__ __forceinline__ uint32_t ekv_fp6_block_exp(float amax) {
  if (amax == 0.f) return 127u;
  const int b = (int)((__float_as_uint(amax) + 0x0FFFFFu) >> 23) - 2;
  return (uint32_t)min(max(b, 1), 254);
}
// the lane's block of the row at `row_ptr` (96 bytes), non-temporal like every K/V row
__device__ __forceinline__ ekv_u6 ekv_fp6_load_block(const char* row_ptr, int sub) {
  const ekv_u2* p = reinterpret_cast<const ekv_u2*>(row_ptr) + sub * 3;
  const ekv_u2 a = __builtin_nontemporal_load(p), b = __builtin_nontemporal_load(p + 1), c = __builtin_nontemporal_load(p + 2);
  return ekv_u6{a[0], a[1], b[0], b[1], c[0], c[1]};
}
__device__ __forceinline__ void ekv_fp6_store_block(char* row_ptr, int sub, const ekv_u6& c) {
  ekv_u2* p = reinterpret_cast<ekv_u2*>(row_ptr) + sub * 3;
  p[0] = ekv_u2{c[0], c[1]}, p[1] = ekv_u2{c[2], c[3]}, p[2] = ekv_u2{c[4], c[5]};
}
// 32 query elements . the 32 codes of a block (the block's scale is the caller's business)
__device__ __forceinline__ float ekv_dot32_fp6(const uint4 (&q)[4], const ekv_u6& c, float acc) {
#if EKV_BF16
  const ekv_h32 k = __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(c, 1.0f);
#else
  const ekv_h32 k = __builtin_amdgcn_cvt_scalef32_pk32_f16_fp6(c, 1.0f);
#endif
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t w[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = EKV_FDOT2(__builtin_bit_cast(ekv_h2, w[j]), ekv_h2{k[8 * i + 2 * j], k[8 * i + 2 * j + 1]}, acc, false);
  }
  return acc;
}
// o[0..32) += p * (codes * scale)
__device__ __forceinline__ void ekv_axpy32_fp6(float p, float scale, const ekv_u6& c, float (&o)[32]) {
  const ekv_f32x f = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(c, scale);
#pragma unroll
  for (int i = 0; i < 32; ++i) o[i] = fmaf(p, f[i], o[i]);
}
// 32 values -> their block under `scale` (a power of two): RNE(x / scale).  v_cvt_scalef32_2xpk16_fp6_f32 interleaves its operands —
// element i of the first lands at position 2i, of the second at 2i + 1 (measured on MI355X) — so they are the even and the odd elements.
// The instruction writes its six result registers while it still reads its 32 sources, and the compiler does not know: left alone it
// places the result inside a source tuple that dies here (v[34:39] over v[28:43] in the split kernel), or over the scale register
// (v[34:39] with the scale in v34 in the conversion kernel): wrong codes, both seen on the part.  The empty asm below keeps the two
// sources and the scale live across the conversion, so the result gets registers of its own.
// What this does and does not guarantee: sources, scale and result are all live right behind the instruction, hence pairwise
// disjoint THERE; nothing stops the compiler from copying a source just before the conversion and converting from the copy, which
// could again die at the instruction.  It does not do that today (every conversion of the kv6 objects and of ekv_kv4 was read in the
// assembly: disjoint operands), and check_rows on every appended and converted row (tests/test_hip_kv6.py) is what would notice.
// The pk32 conversions above need no guard: in this compiler their destination is early-clobber (the machine IR behind instruction
// selection says `early-clobber %dst = V_CVT_SCALEF32_PK32_{F32,F16,BF16}_FP6_e64`), the 2xpk16 one's is not.
__device__ __forceinline__ ekv_u6 ekv_fp6_quant32(const float* f, float scale) {
  ekv_f16x even, odd;
#pragma unroll
  for (int i = 0; i < 16; ++i) even[i] = f[2 * i], odd[i] = f[2 * i + 1];
  const ekv_u6 c = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(even, odd, scale);
  asm volatile("" : : "v"(even), "v"(odd), "v"(scale), "v"(c));
  return c;
}
// 32 source elements (four 16-byte pieces) -> their block: 24 bytes of codes, the exponent byte in `e`
__device__ __forceinline__ ekv_u6 ekv_fp6_quant_block(const uint4* src, uint32_t& e) {
  float f[32];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) amax = fmaxf(amax, ekv_widen8_amax(src[i], f + 8 * i));
  e = ekv_fp6_block_exp(amax);
  return ekv_fp6_quant32(f, ekv_fp4_exp_scale(e));
}

// ---- attention-logit soft-capping (include/easykv_hip.h, "soft-capped logits"): s = cap * tanh(x / cap), x = q.k / sm_div ----------
// The one place the capped logit is computed: every kernel of an EKV_SOFTCAP = 1 build calls ekv_softcap on the fp32 quotient it would
// otherwise have used as the logit, before the mask, the running maximum and the exponent, and everything downstream (softmax, exported
// logits, (m, l, o) partials, row statistics, column sums, scorers and tails) sees only the result.  y = x / cap is the correctly
// rounded quotient.  Three ranges of |y|, each free of the cancellation of 1 - 2 / (1 + e^2y) near 0 (one ulp of 1.0 there is
// cap * 6e-8 on the logit, ten times what torch's own fp32 tanh leaves):
//   |y| < 0.6         tanh y = y + y * w(y), w(y) = y^2 * P(y^2) (degree 5, |error| 3.4e-10 relative); the result is fma(x, w, x), so the
//                     leading term is x itself and no rounding of y or of cap * ... reaches it
//   0.6 <= |y| < 1.6  tanh(a + u) = A + (1 - A^2) * tau / (1 + A * tau) around the nearest of four centres a (|u| <= 0.125), tau = tanh u by
//                     the same polynomial, A = tanh a as an fp32 pair: the correction stays below 0.08, so its roundings stay below half an
//                     ulp of the result
//   |y| >= 1.6        1 - 2 / (1 + e^(2|y|)), the exponent's argument carried as an fp32 pair (2 / (1 + e) < 0.08: v_exp_f32's own ulp is
//                     far below the result's); |y| is clamped to 44 (e^88 is finite), so +-inf gives +-cap
// NaN takes the last branch and propagates; the result is odd in x by construction (|y| and a sign copy) and within 0.75 ulp of
// cap * tanh(x / cap) for a power-of-two cap, within 2 ulp for any other (the rounding of y, as in torch's three ops).  Measured against
// float64 per decade of |y|: profiles/softcap_accuracy.json, tests/test_hip_softcap.py.
#ifndef EKV_SOFTCAP
#define EKV_SOFTCAP 0
#endif
__device__ __forceinline__ float ekv_tanh_w(float u) {      // tanh(u) / u - 1 for |u| <= 0.6
  const float z = u * u;
  float p = 0x1.3719fcp-9f;
  p = fmaf(p, z, -0x1.13a9a0p-7f);
  p = fmaf(p, z, 0x1.64fe24p-6f);
  p = fmaf(p, z, -0x1.ba0dcap-5f);
  p = fmaf(p, z, 0x1.1110f6p-3f);
  p = fmaf(p, z, -0x1.555556p-2f);
  return z * p;
}
__device__ __forceinline__ float ekv_softcap(float x, float cap) {
  const float y = x / cap, ay = fabsf(y);
  if (ay < 0.6f) return fmaf(x, ekv_tanh_w(y), x);
  float t;
  if (ay < 1.6f) {
    // centre a, tanh a = ah + al, 1 - tanh^2 a
    const bool c1 = ay >= 0.85f, c2 = ay >= 1.1f, c3 = ay >= 1.35f;
    const float a = c3 ? 1.475f : (c2 ? 1.225f : (c1 ? 0.975f : 0.725f));
    const float ah = c3 ? 0x1.cd11e0p-1f : (c2 ? 0x1.aea7aap-1f : (c1 ? 0x1.807516p-1f : 0x1.3d703cp-1f));
    const float al = c3 ? -0x1.470dbcp-26f : (c2 ? -0x1.1e7b62p-26f : (c1 ? -0x1.b0c960p-31f : -0x1.85a524p-26f));
    const float b = c3 ? 0x1.832d40p-3f : (c2 ? 0x1.2b8854p-2f : (c1 ? 0x1.bea088p-2f : 0x1.3b306ep-1f));
    const float u = ay - a;      // (exact: both in [0.6, 1.6))
    const float tau = fmaf(u, ekv_tanh_w(u), u);
    t = ah + (al + (tau * b) / fmaf(ah, tau, 1.f));
  } else {
    const float ac = ay > 44.f ? 44.f : ay;      // (NaN stays NaN)
    const float k = 2.f * EKV_LOG2E, kl = (float)(2.0 * 1.4426950408889634 - (double)(2.f * EKV_LOG2E));
    const float eh = ac * k;
    const float el = fmaf(ac, kl, fmaf(ac, k, -eh));      // the argument's low part: 2 |y| log2 e = eh + el
    const float e0 = exp2f(eh);
    const float e = fmaf(e0, el * 0.6931471805599453f, e0);
    t = 1.f - 2.f / (1.f + e);
  }
  return cap * copysignf(t, y);
}
// The logit of a (row, query head) from its dot product: the quotient, capped in the EKV_SOFTCAP builds (decode kernels)
#if EKV_SOFTCAP
#define EKV_LOGIT(acc, a) ekv_softcap((acc) / (a).sm_div, (a).softcap)
#else
#define EKV_LOGIT(acc, a) ((acc) / (a).sm_div)
#endif

// ---- attention sinks (include/easykv_hip.h, "attention sinks"): one learned logit a per query head joins every softmax as a virtual key
// with value 0 ------------------------------------------------------------------------------------------------------------------------
// EKV_SINK = 1 (the EKV_*_SINK lines of the manifest) builds the kernels that take the sinks [n_layers][n_q_heads] (fp32, indexed by bank
// layer) as their LAST kernel argument; EKV_SINK_ONLY(...) spells what exists only in those builds — a parameter, an argument — and
// vanishes everywhere else, so every other instance keeps its tokens.  Every (m, l) that leaves a sink kernel carries the virtual key:
// the decode stream folds it into the online state of the lane group that scores the appended row (ekv_sink_fold: once per query head),
// the chunk kernel seeds the running (m, l) of the first key half of the first split with (a, 1).  Partials, folds, row statistics and
// the statistics pass then have it, and only the places that rebuild the sum of exponentials from a logits row (the decode tails) add
// exp(a - M) themselves.
#if defined(EKV_WINDOW) && EKV_WINDOW == 2 && !defined(EKV_SINK)
#define EKV_SINK 1      // (-DEKV_WINDOW=2, the EKV_*_SINK_WIN lines of the manifest: sliding windows AND sinks, see below)
#endif
#ifndef EKV_SINK
#define EKV_SINK 0
#endif
#if EKV_SINK
#define EKV_SINK_ONLY(...) __VA_ARGS__
#else
#define EKV_SINK_ONLY(...)
#endif
// one more key, of logit a and value 0, for an online-softmax state (m may still be -inf; a is finite)
template <int N>
__device__ __forceinline__ void ekv_sink_fold(float a, float& m, float& l, float (&o)[N]) {
  const float mn = fmaxf(m, a);
  const float alpha = m == EKV_NEG_INF ? 0.f : exp2f((m - mn) * EKV_LOG2E);
  l = l * alpha + exp2f((a - mn) * EKV_LOG2E);
#pragma unroll
  for (int i = 0; i < N; ++i) o[i] *= alpha;
  m = mn;
}

// ---- sliding-window masking (include/easykv_hip.h, "sliding windows"): every physical K/V row carries the token position it was appended
// at (tok_pos [n_layers][H][cap], indexed by physical row like a row scale), and a key whose position lies W_l or more behind the query's
// is masked: logit -inf before the maximum, like a causally masked one, but the row stays live -----------------------------------------
// EKV_WINDOW != 0 (the EKV_*_WIN lines of the manifest; orthogonal to EKV_SINK) builds the kernels that take EkvWinArgs (ekv_kernels.h)
// as their LAST kernel argument, behind the sinks where both are on; EKV_WIN_ONLY(...) spells what exists only in those builds.
// EKV_WINDOW = 2 (the EKV_*_SINK_WIN lines) is EKV_WINDOW = 1 with EKV_SINK = 1, spelled as one switch: the list of objects compiled
// with the sink switch itself is the sink family's own.
#ifndef EKV_WINDOW
#define EKV_WINDOW 0
#endif
#if EKV_WINDOW
#define EKV_WIN_ONLY(...) __VA_ARGS__
#else
#define EKV_WIN_ONLY(...)
#endif
// is the key appended at token position p_k masked for the query at p_q under window w (w = 0: no window; p_k <= p_q)
__device__ __forceinline__ bool ekv_win_masked(int p_q, int p_k, int w) { return w > 0 && p_q - p_k >= w; }

// f32 -> one 16-bit output element, rounded to nearest even (bf16: v_cvt_pk_bf16_f32, NaN kept), as the __half the row pointers hold
__device__ __forceinline__ __half ekv_to_e(float x) {
#if EKV_BF16
  return __builtin_bit_cast(__half, (__bf16)x);
#else
  return __float2half(x);
#endif
}
__device__ __forceinline__ __half2 ekv_to_e2(float x, float y) {
#if EKV_BF16
  return __builtin_bit_cast(__half2, ekv_h2{(__bf16)x, (__bf16)y});
#else
  return __floats2half2_rn(x, y);
#endif
}

__device__ __forceinline__ float ekv_wave_max(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
  return x;
}
__device__ __forceinline__ float ekv_wave_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
__device__ __forceinline__ unsigned long long ekv_wave_min_u64(unsigned long long x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long y = __shfl_xor(x, off, 64);
    x = y < x ? y : x;
  }
  return x;
}

// Order-preserving float -> uint32 key (ascending); every NaN maps to the largest key, which is how
// torch.topk(largest=False) ranks NaN.
__device__ __forceinline__ uint32_t ekv_fkey(float x) {
  if (x != x) return 0xFFFFFFFFu;
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Fold the key-range-split partials (m, l, o[D]) of one query row into o[d] / l.  All loads of a pass are issued
// together (BATCH splits per round trip): a naive loop serialises one L2 round trip per split (~10 us for 17 splits).
// `mm` / `ls` return the row's softmax statistics (max logit, sum of exp(logit - max)) over all splits.
template <int BATCH = 32>
__device__ __forceinline__ float ekv_fold_partials(const float* p0, int n_split, int PS, int d, float& mm, float& ls) {
  mm = EKV_NEG_INF;
  ls = 0.f;
  float os = 0.f;
  for (int s0 = 0; s0 < n_split; s0 += BATCH) {
    float mv[BATCH], lv[BATCH], ov[BATCH];
#pragma unroll
    for (int i = 0; i < BATCH; ++i) {
      const bool ok = s0 + i < n_split;
      const float* p = p0 + (size_t)(ok ? s0 + i : 0) * PS;
      const float pm = p[0], pl = p[1], po = p[2 + d];   // unconditional loads (clamped pointer), masked afterwards
      mv[i] = ok ? pm : EKV_NEG_INF;
      lv[i] = ok ? pl : 0.f;
      ov[i] = ok ? po : 0.f;
    }
    float mb = mm;
#pragma unroll
    for (int i = 0; i < BATCH; ++i) mb = fmaxf(mb, mv[i]);
    const float rescale = (mm == EKV_NEG_INF) ? 0.f : exp2f((mm - mb) * EKV_LOG2E);
    ls *= rescale;
    os *= rescale;
#pragma unroll
    for (int i = 0; i < BATCH; ++i) {
      const float w = (mv[i] == EKV_NEG_INF) ? 0.f : exp2f((mv[i] - mb) * EKV_LOG2E);
      ls += lv[i] * w;
      os += ov[i] * w;
    }
    mm = mb;
  }
  return os / ls;
}

template <int BATCH = 32>
__device__ __forceinline__ float ekv_fold_partials(const float* p0, int n_split, int PS, int d) {
  float mm, ls;
  return ekv_fold_partials<BATCH>(p0, n_split, PS, d, mm, ls);
}

// Batch = loads issued together per round trip.  Masked entries of a batch add exact zeros, so any batch that covers all
// partials gives the same result; a batch much wider than n_split only wastes clamped loads (C3: 32-wide batches over 8
// partials were 65 % of its scorer).  Batches are capped at 16 (8 for 1024-thread blocks): a 32-wide batch keeps 96 values live,
// and under a 512-thread launch bound (128 VGPRs) hipcc then serialises it into one exposed round trip PER SPLIT — 17 of them,
// 8.5 of the 19 us of the per-layer decode scorer.
template <int MAXB = 16>
__device__ __forceinline__ float ekv_fold_partials_auto(const float* p0, int n_split, int PS, int d, float& mm, float& ls) {
  if (MAXB <= 8 || n_split <= 8) return ekv_fold_partials<8>(p0, n_split, PS, d, mm, ls);
  if (n_split <= 16 || n_split > 24) return ekv_fold_partials<16>(p0, n_split, PS, d, mm, ls);
  return ekv_fold_partials<24>(p0, n_split, PS, d, mm, ls);   // 17..24 partials (decode, T ~ 2k: 17 splits) in ONE round trip
}
template <int MAXB = 16>
__device__ __forceinline__ float ekv_fold_partials_auto(const float* p0, int n_split, int PS, int d) {
  float mm, ls;
  return ekv_fold_partials_auto<MAXB>(p0, n_split, PS, d, mm, ls);
}

// Agent-scope store of a partial that ANOTHER workgroup of the same launch will read (global_store ... sc1: written through to the
// memory side, where the reader's sc1 loads find it).
__device__ __forceinline__ void ekv_store_sc1(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The same fold over partials written by OTHER workgroups of the same launch (in-kernel fold by the last-arriving split): the
// loads are buffer loads with the sc1 cache policy (agent scope: served by memory-side caches, never by this CU's L1 or a stale
// line) from a wave-UNIFORM descriptor + per-lane offsets, so a batch still goes out as one round trip.  (__hip_atomic_load is
// issued one load at a time with a wait behind each: 51 serialised round trips made the fold cost 25 us; a descriptor built
// from a per-lane pointer makes hipcc wrap every load in a waterfall loop.)  Arithmetic identical to ekv_fold_partials.
template <int BATCH>
__device__ __forceinline__ float ekv_fold_partials_buf(__amdgpu_buffer_rsrc_t rsrc, unsigned row_off, int n_split, int PS, int d) {
  float mm = EKV_NEG_INF, ls = 0.f, os = 0.f;
  for (int s0 = 0; s0 < n_split; s0 += BATCH) {
    float mv[BATCH], lv[BATCH], ov[BATCH];
#pragma unroll
    for (int i = 0; i < BATCH; ++i) {
      const bool ok = s0 + i < n_split;
      const unsigned off = (row_off + (unsigned)(ok ? s0 + i : 0) * (unsigned)PS) * 4u;
      const float pm = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 16));
      const float pl = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off + 4u, 0, 16));
      const float po = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off + 8u + 4u * (unsigned)d, 0, 16));
      mv[i] = ok ? pm : EKV_NEG_INF;
      lv[i] = ok ? pl : 0.f;
      ov[i] = ok ? po : 0.f;
    }
    float mb = mm;
#pragma unroll
    for (int i = 0; i < BATCH; ++i) mb = fmaxf(mb, mv[i]);
    const float rescale = (mm == EKV_NEG_INF) ? 0.f : exp2f((mm - mb) * EKV_LOG2E);
    ls *= rescale;
    os *= rescale;
#pragma unroll
    for (int i = 0; i < BATCH; ++i) {
      const float w = (mv[i] == EKV_NEG_INF) ? 0.f : exp2f((mv[i] - mb) * EKV_LOG2E);
      ls += lv[i] * w;
      os += ov[i] * w;
    }
    mm = mb;
  }
  return os / ls;
}
__device__ __forceinline__ float ekv_fold_partials_buf_auto(__amdgpu_buffer_rsrc_t rsrc, unsigned row_off, int n_split, int PS, int d) {
  if (n_split <= 8) return ekv_fold_partials_buf<8>(rsrc, row_off, n_split, PS, d);       // (same batch choice as
  if (n_split <= 16 || n_split > 24) return ekv_fold_partials_buf<16>(rsrc, row_off, n_split, PS, d);   //  ekv_fold_partials_auto<16>)
  return ekv_fold_partials_buf<24>(rsrc, row_off, n_split, PS, d);
}

// Barrier that only orders LDS traffic: global loads of the next super-tile stay in flight across it
// (__syncthreads() would drain vmcnt(0) whenever a global store may be pending).
__device__ __forceinline__ void ekv_lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
