// The conversion unit of the MX block formats (MXFP4 first; MXFP6, "kv6", then FP8 keys with MXFP4 values, "kv84", and 16-bit keys with MXFP4
// values, "kv164": the same launch shape around another block).
// MXFP4 K/V storage ("kv4", include/easykv_hip.h; head_dim 128): conversion of a 16-bit bank to e2m1 codes + E8M0 block exponents at the
// same physical rows, and the inverse.  One pass, 16-byte loads, one lane per 32-element block (four lanes per row): a lane reads its
// block's 64 source bytes, takes the exponent from the bits of the block maximum and packs the codes with v_cvt_scalef32_pk_fp4_f32.
#include "ekv_common.h"
#include "ekv_kernels.h"

namespace {

constexpr int kBlocks = 4;      // blocks (lanes) per row at head_dim 128

// block b of the launch -> index of physical row (layer_begin + r / (H * extent), head, row) in a [layers][H][cap] array; r = b / 4
__device__ __forceinline__ size_t kv4_row(long long r, int n_kv_heads, int cap, int layer_begin, int extent) {
  const long long lh = r / extent;
  return ((size_t)layer_begin * n_kv_heads + (size_t)lh) * cap + (size_t)(r % extent);
}

// BF: the source elements are bf16.  (Both element types in one unit: the widening is spelled out instead of going through ekv_e.)
template <bool BF>
__global__ void __launch_bounds__(256) ekv_kv4_quantize_kernel(const uint4* __restrict__ k, const uint4* __restrict__ v, uint4* __restrict__ kc,
                                                               uint4* __restrict__ vc, uint8_t* __restrict__ ke, uint8_t* __restrict__ ve,
                                                               int n_kv_heads, int cap, int layer_begin, int extent, long long n_rows) {
  const int sub = threadIdx.x % kBlocks;
  const long long r = (long long)blockIdx.x * (256 / kBlocks) + threadIdx.x / kBlocks;
  if (r >= n_rows) return;
  const size_t row = kv4_row(r, n_kv_heads, cap, layer_begin, extent);
  auto one = [&](const uint4* src, uint4* codes, uint8_t* exps) {
    float f[32];
    float amax = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint4 x = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(src + row * 16) + sub * 4 + p));
      const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float a, b;
        if (BF) {
          a = __uint_as_float(w[i] << 16);
          b = __uint_as_float(w[i] & 0xFFFF0000u);
        } else {
          typedef _Float16 h2 __attribute__((ext_vector_type(2)));
          const h2 h = __builtin_bit_cast(h2, w[i]);
          a = (float)h[0];
          b = (float)h[1];
        }
        f[8 * p + 2 * i] = a;
        f[8 * p + 2 * i + 1] = b;
        amax = fmaxf(amax, fmaxf(fabsf(a), fabsf(b)));
      }
    }
    const uint32_t e = ekv_fp4_block_exp(amax);
    const float s = ekv_fp4_exp_scale(e);
    codes[row * kBlocks + sub] = uint4{ekv_fp4_quant8(f, s), ekv_fp4_quant8(f + 8, s), ekv_fp4_quant8(f + 16, s), ekv_fp4_quant8(f + 24, s)};
    exps[row * kBlocks + sub] = (uint8_t)e;
  };
  one(k, kc, ke);
  one(v, vc, ve);
}

// OUT: 0 fp16, 1 bf16, 2 fp32.  One thread per block; out is dense [rows][128].
template <int OUT>
__global__ void __launch_bounds__(256) ekv_kv4_dequantize_kernel(const uint4* __restrict__ kc, const uint4* __restrict__ vc, const uint8_t* __restrict__ ke,
                                                                 const uint8_t* __restrict__ ve, void* __restrict__ k_out, void* __restrict__ v_out,
                                                                 int n_kv_heads, int cap, int layer_begin, int extent, long long n_rows) {
  const int sub = threadIdx.x % kBlocks;
  const long long r = (long long)blockIdx.x * (256 / kBlocks) + threadIdx.x / kBlocks;
  if (r >= n_rows) return;
  const size_t row = kv4_row(r, n_kv_heads, cap, layer_begin, extent);
  auto one = [&](const uint4* codes, const uint8_t* exps, void* out) {
    const uint4 c = codes[row * kBlocks + sub];
    const float s = ekv_fp4_exp_scale(exps[row * kBlocks + sub]);
    float f[32];
    ekv_fp4_widen8(c.x, s, f), ekv_fp4_widen8(c.y, s, f + 8), ekv_fp4_widen8(c.z, s, f + 16), ekv_fp4_widen8(c.w, s, f + 24);
    const size_t o = ((size_t)r * kBlocks + sub) * 32;
    if (OUT == 2) {
      float4* p = reinterpret_cast<float4*>(static_cast<float*>(out) + o);
#pragma unroll
      for (int i = 0; i < 8; ++i) p[i] = float4{f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]};
    } else {
      uint32_t w[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (OUT == 1) {
          typedef __bf16 b2 __attribute__((ext_vector_type(2)));
          w[i] = __builtin_bit_cast(uint32_t, b2{(__bf16)f[2 * i], (__bf16)f[2 * i + 1]});
        } else {
          w[i] = __builtin_bit_cast(uint32_t, __floats2half2_rn(f[2 * i], f[2 * i + 1]));
        }
      }
      uint4* p = reinterpret_cast<uint4*>(static_cast<uint16_t*>(out) + o);
#pragma unroll
      for (int i = 0; i < 4; ++i) p[i] = uint4{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
    }
  };
  one(kc, ke, k_out);
  one(vc, ve, v_out);
}

inline dim3 kv4_grid(long long n_rows) { return dim3((unsigned)((n_rows + 256 / kBlocks - 1) / (256 / kBlocks))); }

// ---- MXFP6 ("kv6"): one lane per 32-element block as above; a block is 24 bytes of e2m3 codes (v_cvt_scalef32_2xpk16_fp6_f32 /
// v_cvt_scalef32_pk32_f32_fp6), a row 96 bytes, the exponent plane is kv4's
template <bool BF>
__global__ void __launch_bounds__(256) ekv_kv6_quantize_kernel(const uint4* __restrict__ k, const uint4* __restrict__ v, char* __restrict__ kc,
                                                               char* __restrict__ vc, uint8_t* __restrict__ ke, uint8_t* __restrict__ ve,
                                                               int n_kv_heads, int cap, int layer_begin, int extent, long long n_rows) {
  const int sub = threadIdx.x % kBlocks;
  const long long r = (long long)blockIdx.x * (256 / kBlocks) + threadIdx.x / kBlocks;
  if (r >= n_rows) return;
  const size_t row = kv4_row(r, n_kv_heads, cap, layer_begin, extent);
  auto one = [&](const uint4* src, char* codes, uint8_t* exps) {
    float f[32];
    float amax = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint4 x = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(src + row * 16) + sub * 4 + p));
      const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float a, b;
        if (BF) {
          a = __uint_as_float(w[i] << 16);
          b = __uint_as_float(w[i] & 0xFFFF0000u);
        } else {
          typedef _Float16 h2 __attribute__((ext_vector_type(2)));
          const h2 h = __builtin_bit_cast(h2, w[i]);
          a = (float)h[0];
          b = (float)h[1];
        }
        f[8 * p + 2 * i] = a;
        f[8 * p + 2 * i + 1] = b;
        amax = fmaxf(amax, fmaxf(fabsf(a), fabsf(b)));
      }
    }
    const uint32_t e = ekv_fp6_block_exp(amax);
    ekv_fp6_store_block(codes + row * 96, sub, ekv_fp6_quant32(f, ekv_fp4_exp_scale(e)));
    exps[row * kBlocks + sub] = (uint8_t)e;
  };
  one(k, kc, ke);
  one(v, vc, ve);
}

// OUT: 0 fp16, 1 bf16, 2 fp32.  One thread per block; out is dense [rows][128].
template <int OUT>
__global__ void __launch_bounds__(256) ekv_kv6_dequantize_kernel(const char* __restrict__ kc, const char* __restrict__ vc, const uint8_t* __restrict__ ke,
                                                                 const uint8_t* __restrict__ ve, void* __restrict__ k_out, void* __restrict__ v_out,
                                                                 int n_kv_heads, int cap, int layer_begin, int extent, long long n_rows) {
  const int sub = threadIdx.x % kBlocks;
  const long long r = (long long)blockIdx.x * (256 / kBlocks) + threadIdx.x / kBlocks;
  if (r >= n_rows) return;
  const size_t row = kv4_row(r, n_kv_heads, cap, layer_begin, extent);
  auto one = [&](const char* codes, const uint8_t* exps, void* out) {
    const ekv_u2* cp = reinterpret_cast<const ekv_u2*>(codes + row * 96) + sub * 3;
    const ekv_u2 c0 = cp[0], c1 = cp[1], c2 = cp[2];
    const ekv_f32x f = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(ekv_u6{c0[0], c0[1], c1[0], c1[1], c2[0], c2[1]},
                                                                   ekv_fp4_exp_scale(exps[row * kBlocks + sub]));
    const size_t o = ((size_t)r * kBlocks + sub) * 32;
    if (OUT == 2) {
      float4* p = reinterpret_cast<float4*>(static_cast<float*>(out) + o);
#pragma unroll
      for (int i = 0; i < 8; ++i) p[i] = float4{f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]};
    } else {
      uint32_t w[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (OUT == 1) {
          typedef __bf16 b2 __attribute__((ext_vector_type(2)));
          w[i] = __builtin_bit_cast(uint32_t, b2{(__bf16)f[2 * i], (__bf16)f[2 * i + 1]});
        } else {
          w[i] = __builtin_bit_cast(uint32_t, __floats2half2_rn(f[2 * i], f[2 * i + 1]));
        }
      }
      uint4* p = reinterpret_cast<uint4*>(static_cast<uint16_t*>(out) + o);
#pragma unroll
      for (int i = 0; i < 4; ++i) p[i] = uint4{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
    }
  };
  one(kc, ke, k_out);
  one(vc, ve, v_out);
}

// ---- FP8 keys with MXFP4 values ("kv84"): one lane per 32 elements as above.  K: the kv8 rule — the row maximum over the row's four
// lanes, one fp32 scale per row, 32 e4m3 codes per lane (ekv_common.h: ekv_fp8_row_scale / ekv_fp8_quant4, what ekv_kv8.hip runs).
// V: the kv4 rule — the lane's block, as ekv_kv4_quantize_kernel packs it.
template <bool BF>
__global__ void __launch_bounds__(256) ekv_kv84_quantize_kernel(const uint4* __restrict__ k, const uint4* __restrict__ v, uint4* __restrict__ kc,
                                                                uint4* __restrict__ vc, float* __restrict__ ks, uint8_t* __restrict__ ve,
                                                                int n_kv_heads, int cap, int layer_begin, int extent, long long n_rows) {
  const int sub = threadIdx.x % kBlocks;
  const long long r = (long long)blockIdx.x * (256 / kBlocks) + threadIdx.x / kBlocks;
  if (r >= n_rows) return;      // (whole rows: the four lanes of a row's group leave together)
  const size_t row = kv4_row(r, n_kv_heads, cap, layer_begin, extent);
  auto widen = [&](const uint4* src, float* f) {
    float amax = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint4 x = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(src + row * 16) + sub * 4 + p));
      const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float a, b;
        if (BF) {
          a = __uint_as_float(w[i] << 16);
          b = __uint_as_float(w[i] & 0xFFFF0000u);
        } else {
          typedef _Float16 h2 __attribute__((ext_vector_type(2)));
          const h2 h = __builtin_bit_cast(h2, w[i]);
          a = (float)h[0];
          b = (float)h[1];
        }
        f[8 * p + 2 * i] = a;
        f[8 * p + 2 * i + 1] = b;
        amax = fmaxf(amax, fmaxf(fabsf(a), fabsf(b)));
      }
    }
    return amax;
  };
  float f[32];
  const float sk = ekv_fp8_row_scale(ekv_group_max<kBlocks>(widen(k, f)));
  uint32_t c[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) c[i] = ekv_fp8_quant4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3], sk);
  kc[(row * kBlocks + sub) * 2] = uint4{c[0], c[1], c[2], c[3]};
  kc[(row * kBlocks + sub) * 2 + 1] = uint4{c[4], c[5], c[6], c[7]};
  if (sub == 0) ks[row] = sk;
  const uint32_t e = ekv_fp4_block_exp(widen(v, f));
  const float s = ekv_fp4_exp_scale(e);
  vc[row * kBlocks + sub] = uint4{ekv_fp4_quant8(f, s), ekv_fp4_quant8(f + 8, s), ekv_fp4_quant8(f + 16, s), ekv_fp4_quant8(f + 24, s)};
  ve[row * kBlocks + sub] = (uint8_t)e;
}

// OUT: 0 fp16, 1 bf16, 2 fp32.  One thread per 32 elements; out is dense [rows][128].
template <int OUT>
__global__ void __launch_bounds__(256) ekv_kv84_dequantize_kernel(const uint4* __restrict__ kc, const uint4* __restrict__ vc, const float* __restrict__ ks,
                                                                  const uint8_t* __restrict__ ve, void* __restrict__ k_out, void* __restrict__ v_out,
                                                                  int n_kv_heads, int cap, int layer_begin, int extent, long long n_rows) {
  const int sub = threadIdx.x % kBlocks;
  const long long r = (long long)blockIdx.x * (256 / kBlocks) + threadIdx.x / kBlocks;
  if (r >= n_rows) return;
  const size_t row = kv4_row(r, n_kv_heads, cap, layer_begin, extent);
  auto store = [&](const float* f, void* out) {
    const size_t o = ((size_t)r * kBlocks + sub) * 32;
    if (OUT == 2) {
      float4* p = reinterpret_cast<float4*>(static_cast<float*>(out) + o);
#pragma unroll
      for (int i = 0; i < 8; ++i) p[i] = float4{f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]};
    } else {
      uint32_t w[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (OUT == 1) {
          typedef __bf16 b2 __attribute__((ext_vector_type(2)));
          w[i] = __builtin_bit_cast(uint32_t, b2{(__bf16)f[2 * i], (__bf16)f[2 * i + 1]});
        } else {
          w[i] = __builtin_bit_cast(uint32_t, __floats2half2_rn(f[2 * i], f[2 * i + 1]));
        }
      }
      uint4* p = reinterpret_cast<uint4*>(static_cast<uint16_t*>(out) + o);
#pragma unroll
      for (int i = 0; i < 4; ++i) p[i] = uint4{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
    }
  };
  float f[32];
  const uint4 k0 = kc[(row * kBlocks + sub) * 2], k1 = kc[(row * kBlocks + sub) * 2 + 1];
  const uint32_t kw[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
  const float sk = ks[row];
#pragma unroll
  for (int i = 0; i < 8; ++i) ekv_fp8_widen4(kw[i], f + 4 * i);
#pragma unroll
  for (int i = 0; i < 32; ++i) f[i] *= sk;
  store(f, k_out);
  const uint4 c = vc[row * kBlocks + sub];
  const float s = ekv_fp4_exp_scale(ve[row * kBlocks + sub]);
  ekv_fp4_widen8(c.x, s, f), ekv_fp4_widen8(c.y, s, f + 8), ekv_fp4_widen8(c.z, s, f + 16), ekv_fp4_widen8(c.w, s, f + 24);
  store(f, v_out);
}

// ---- 16-bit keys with MXFP4 values ("kv164"): the V plane alone, one lane per 32-element block as above — the block of
// ekv_kv4_quantize_kernel's V side, so the planes are its V planes byte for byte.  K is neither read nor written.
template <bool BF>
__global__ void __launch_bounds__(256) ekv_kv164_quantize_kernel(const uint4* __restrict__ v, uint4* __restrict__ vc, uint8_t* __restrict__ ve,
                                                                 int n_kv_heads, int cap, int layer_begin, int extent, long long n_rows) {
  const int sub = threadIdx.x % kBlocks;
  const long long r = (long long)blockIdx.x * (256 / kBlocks) + threadIdx.x / kBlocks;
  if (r >= n_rows) return;
  const size_t row = kv4_row(r, n_kv_heads, cap, layer_begin, extent);
  float f[32];
  float amax = 0.f;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const uint4 x = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(v + row * 16) + sub * 4 + p));
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float a, b;
      if (BF) {
        a = __uint_as_float(w[i] << 16);
        b = __uint_as_float(w[i] & 0xFFFF0000u);
      } else {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const h2 h = __builtin_bit_cast(h2, w[i]);
        a = (float)h[0];
        b = (float)h[1];
      }
      f[8 * p + 2 * i] = a;
      f[8 * p + 2 * i + 1] = b;
      amax = fmaxf(amax, fmaxf(fabsf(a), fabsf(b)));
    }
  }
  const uint32_t e = ekv_fp4_block_exp(amax);
  const float s = ekv_fp4_exp_scale(e);
  vc[row * kBlocks + sub] = uint4{ekv_fp4_quant8(f, s), ekv_fp4_quant8(f + 8, s), ekv_fp4_quant8(f + 16, s), ekv_fp4_quant8(f + 24, s)};
  ve[row * kBlocks + sub] = (uint8_t)e;
}

// OUT: 0 fp16, 1 bf16, 2 fp32.  One thread per block; v_out is dense [rows][128].
template <int OUT>
__global__ void __launch_bounds__(256) ekv_kv164_dequantize_kernel(const uint4* __restrict__ vc, const uint8_t* __restrict__ ve, void* __restrict__ v_out,
                                                                   int n_kv_heads, int cap, int layer_begin, int extent, long long n_rows) {
  const int sub = threadIdx.x % kBlocks;
  const long long r = (long long)blockIdx.x * (256 / kBlocks) + threadIdx.x / kBlocks;
  if (r >= n_rows) return;
  const size_t row = kv4_row(r, n_kv_heads, cap, layer_begin, extent);
  const uint4 c = vc[row * kBlocks + sub];
  const float s = ekv_fp4_exp_scale(ve[row * kBlocks + sub]);
  float f[32];
  ekv_fp4_widen8(c.x, s, f), ekv_fp4_widen8(c.y, s, f + 8), ekv_fp4_widen8(c.z, s, f + 16), ekv_fp4_widen8(c.w, s, f + 24);
  const size_t o = ((size_t)r * kBlocks + sub) * 32;
  if (OUT == 2) {
    float4* p = reinterpret_cast<float4*>(static_cast<float*>(v_out) + o);
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = float4{f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]};
  } else {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (OUT == 1) {
        typedef __bf16 b2 __attribute__((ext_vector_type(2)));
        w[i] = __builtin_bit_cast(uint32_t, b2{(__bf16)f[2 * i], (__bf16)f[2 * i + 1]});
      } else {
        w[i] = __builtin_bit_cast(uint32_t, __floats2half2_rn(f[2 * i], f[2 * i + 1]));
      }
    }
    uint4* p = reinterpret_cast<uint4*>(static_cast<uint16_t*>(v_out) + o);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = uint4{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
  }
}

}  // namespace

hipError_t ekv_launch_kv4_quantize(const ekv_bank* bank, const ekv_kv4* q4, bool src_bf16, int layer_begin, int layer_count, int extent,
                                   hipStream_t s) {
  if (bank->head_dim != 128) return hipErrorInvalidValue;
  const long long n_rows = (long long)layer_count * bank->n_kv_heads * extent;
  if (n_rows == 0) return hipSuccess;
#define EKV_KV4_Q(BF)                                                                                                           \
  hipLaunchKernelGGL((ekv_kv4_quantize_kernel<BF>), kv4_grid(n_rows), dim3(256), 0, s, static_cast<const uint4*>(bank->k),     \
                     static_cast<const uint4*>(bank->v), static_cast<uint4*>(q4->k_codes), static_cast<uint4*>(q4->v_codes),   \
                     q4->k_exp, q4->v_exp, bank->n_kv_heads, bank->cap, layer_begin, extent, n_rows)
  if (src_bf16) EKV_KV4_Q(true); else EKV_KV4_Q(false);
#undef EKV_KV4_Q
  return hipGetLastError();
}

hipError_t ekv_launch_kv4_dequantize(const ekv_bank* bank, const ekv_kv4* q4, int out_kind, int layer_begin, int layer_count, int extent,
                                     void* k_out, void* v_out, hipStream_t s) {
  if (bank->head_dim != 128) return hipErrorInvalidValue;
  const long long n_rows = (long long)layer_count * bank->n_kv_heads * extent;
  if (n_rows == 0) return hipSuccess;
#define EKV_KV4_DQ(OUT)                                                                                                         \
  hipLaunchKernelGGL((ekv_kv4_dequantize_kernel<OUT>), kv4_grid(n_rows), dim3(256), 0, s, static_cast<const uint4*>(q4->k_codes), \
                     static_cast<const uint4*>(q4->v_codes), q4->k_exp, q4->v_exp, k_out, v_out, bank->n_kv_heads, bank->cap,   \
                     layer_begin, extent, n_rows)
  switch (out_kind) {
    case 0: EKV_KV4_DQ(0); break;
    case 1: EKV_KV4_DQ(1); break;
    case 2: EKV_KV4_DQ(2); break;
    default: return hipErrorInvalidValue;
  }
#undef EKV_KV4_DQ
  return hipGetLastError();
}

hipError_t ekv_launch_kv6_quantize(const ekv_bank* bank, const ekv_kv6* q6, bool src_bf16, int layer_begin, int layer_count, int extent,
                                   hipStream_t s) {
  if (bank->head_dim != 128) return hipErrorInvalidValue;
  const long long n_rows = (long long)layer_count * bank->n_kv_heads * extent;
  if (n_rows == 0) return hipSuccess;
#define EKV_KV6_Q(BF)                                                                                                           \
  hipLaunchKernelGGL((ekv_kv6_quantize_kernel<BF>), kv4_grid(n_rows), dim3(256), 0, s, static_cast<const uint4*>(bank->k),     \
                     static_cast<const uint4*>(bank->v), static_cast<char*>(q6->k_codes), static_cast<char*>(q6->v_codes),     \
                     q6->k_exp, q6->v_exp, bank->n_kv_heads, bank->cap, layer_begin, extent, n_rows)
  if (src_bf16) EKV_KV6_Q(true); else EKV_KV6_Q(false);
#undef EKV_KV6_Q
  return hipGetLastError();
}

hipError_t ekv_launch_kv6_dequantize(const ekv_bank* bank, const ekv_kv6* q6, int out_kind, int layer_begin, int layer_count, int extent,
                                     void* k_out, void* v_out, hipStream_t s) {
  if (bank->head_dim != 128) return hipErrorInvalidValue;
  const long long n_rows = (long long)layer_count * bank->n_kv_heads * extent;
  if (n_rows == 0) return hipSuccess;
#define EKV_KV6_DQ(OUT)                                                                                                         \
  hipLaunchKernelGGL((ekv_kv6_dequantize_kernel<OUT>), kv4_grid(n_rows), dim3(256), 0, s, static_cast<const char*>(q6->k_codes), \
                     static_cast<const char*>(q6->v_codes), q6->k_exp, q6->v_exp, k_out, v_out, bank->n_kv_heads, bank->cap,    \
                     layer_begin, extent, n_rows)
  switch (out_kind) {
    case 0: EKV_KV6_DQ(0); break;
    case 1: EKV_KV6_DQ(1); break;
    case 2: EKV_KV6_DQ(2); break;
    default: return hipErrorInvalidValue;
  }
#undef EKV_KV6_DQ
  return hipGetLastError();
}

hipError_t ekv_launch_kv84_quantize(const ekv_bank* bank, const ekv_kv84* q84, bool src_bf16, int layer_begin, int layer_count, int extent,
                                    hipStream_t s) {
  if (bank->head_dim != 128) return hipErrorInvalidValue;
  const long long n_rows = (long long)layer_count * bank->n_kv_heads * extent;
  if (n_rows == 0) return hipSuccess;
#define EKV_KV84_Q(BF)                                                                                                          \
  hipLaunchKernelGGL((ekv_kv84_quantize_kernel<BF>), kv4_grid(n_rows), dim3(256), 0, s, static_cast<const uint4*>(bank->k),    \
                     static_cast<const uint4*>(bank->v), static_cast<uint4*>(q84->k_codes), static_cast<uint4*>(q84->v_codes), \
                     q84->k_scale, q84->v_exp, bank->n_kv_heads, bank->cap, layer_begin, extent, n_rows)
  if (src_bf16) EKV_KV84_Q(true); else EKV_KV84_Q(false);
#undef EKV_KV84_Q
  return hipGetLastError();
}

hipError_t ekv_launch_kv84_dequantize(const ekv_bank* bank, const ekv_kv84* q84, int out_kind, int layer_begin, int layer_count, int extent,
                                      void* k_out, void* v_out, hipStream_t s) {
  if (bank->head_dim != 128) return hipErrorInvalidValue;
  const long long n_rows = (long long)layer_count * bank->n_kv_heads * extent;
  if (n_rows == 0) return hipSuccess;
#define EKV_KV84_DQ(OUT)                                                                                                         \
  hipLaunchKernelGGL((ekv_kv84_dequantize_kernel<OUT>), kv4_grid(n_rows), dim3(256), 0, s, static_cast<const uint4*>(q84->k_codes), \
                     static_cast<const uint4*>(q84->v_codes), q84->k_scale, q84->v_exp, k_out, v_out, bank->n_kv_heads, bank->cap,  \
                     layer_begin, extent, n_rows)
  switch (out_kind) {
    case 0: EKV_KV84_DQ(0); break;
    case 1: EKV_KV84_DQ(1); break;
    case 2: EKV_KV84_DQ(2); break;
    default: return hipErrorInvalidValue;
  }
#undef EKV_KV84_DQ
  return hipGetLastError();
}

hipError_t ekv_launch_kv164_quantize(const ekv_bank* bank, const ekv_kv164* q164, bool src_bf16, int layer_begin, int layer_count, int extent,
                                     hipStream_t s) {
  if (bank->head_dim != 128) return hipErrorInvalidValue;
  const long long n_rows = (long long)layer_count * bank->n_kv_heads * extent;
  if (n_rows == 0) return hipSuccess;
#define EKV_KV164_Q(BF)                                                                                                        \
  hipLaunchKernelGGL((ekv_kv164_quantize_kernel<BF>), kv4_grid(n_rows), dim3(256), 0, s, static_cast<const uint4*>(bank->v),  \
                     static_cast<uint4*>(q164->v_codes), q164->v_exp, bank->n_kv_heads, bank->cap, layer_begin, extent, n_rows)
  if (src_bf16) EKV_KV164_Q(true); else EKV_KV164_Q(false);
#undef EKV_KV164_Q
  return hipGetLastError();
}

hipError_t ekv_launch_kv164_dequantize(const ekv_bank* bank, const ekv_kv164* q164, int out_kind, int layer_begin, int layer_count, int extent,
                                       void* v_out, hipStream_t s) {
  if (bank->head_dim != 128) return hipErrorInvalidValue;
  const long long n_rows = (long long)layer_count * bank->n_kv_heads * extent;
  if (n_rows == 0) return hipSuccess;
#define EKV_KV164_DQ(OUT)                                                                                                              \
  hipLaunchKernelGGL((ekv_kv164_dequantize_kernel<OUT>), kv4_grid(n_rows), dim3(256), 0, s, static_cast<const uint4*>(q164->v_codes), \
                     q164->v_exp, v_out, bank->n_kv_heads, bank->cap, layer_begin, extent, n_rows)
  switch (out_kind) {
    case 0: EKV_KV164_DQ(0); break;
    case 1: EKV_KV164_DQ(1); break;
    case 2: EKV_KV164_DQ(2); break;
    default: return hipErrorInvalidValue;
  }
#undef EKV_KV164_DQ
  return hipGetLastError();
}
