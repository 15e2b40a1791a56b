// FP8 K/V storage ("kv8", include/easykv_hip.h): conversion of a 16-bit bank to codes + row scales at the same physical rows, and
// the inverse.  One pass, 16-byte loads, one lane group per row (head_dim / 8 lanes: a lane holds 8 source elements = 8 codes).
#include "ekv_common.h"
#include "ekv_kernels.h"

namespace {

// row r of the launch -> element offset of physical row (layer_begin + r / (H * extent), head, row) in a [layers][H][cap] array
__device__ __forceinline__ size_t kv8_row(long long r, int n_kv_heads, int cap, int layer_begin, int extent) {
  const long long lh = r / extent;
  return ((size_t)layer_begin * n_kv_heads + (size_t)lh) * cap + (size_t)(r % extent);
}

// BF: the source elements are bf16.  (Both element types in one unit: the widening is spelled out instead of going through ekv_e.)
template <int D, bool BF>
__global__ void __launch_bounds__(256) ekv_kv8_quantize_kernel(const uint4* __restrict__ k, const uint4* __restrict__ v, uint2* __restrict__ kc,
                                                               uint2* __restrict__ vc, float* __restrict__ ks, float* __restrict__ vs,
                                                               int n_kv_heads, int cap, int layer_begin, int extent, long long n_rows) {
  constexpr int LPR = D / 8;      // 16 (head_dim 128) or 8 (head_dim 64)
  const int sub = threadIdx.x % LPR;
  const long long r = (long long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  const bool live = r < n_rows;      // (whole lane groups: the group reductions below run in every lane)
  const size_t row = kv8_row(live ? r : 0, n_kv_heads, cap, layer_begin, extent);
  auto widen = [](const uint4& x, float* f) {
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (BF) {
        f[2 * i] = __uint_as_float(w[i] << 16);
        f[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
      } else {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const h2 h = __builtin_bit_cast(h2, w[i]);
        f[2 * i] = (float)h[0];
        f[2 * i + 1] = (float)h[1];
      }
      m = fmaxf(m, fmaxf(fabsf(f[2 * i]), fabsf(f[2 * i + 1])));
    }
    return m;
  };
  float kf[8], vf[8];
  const uint4 kx = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(k + row * LPR) + sub));
  const uint4 vx = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(v + row * LPR) + sub));
  const float sk = ekv_fp8_row_scale(ekv_group_max<LPR>(widen(kx, kf)));
  const float sv = ekv_fp8_row_scale(ekv_group_max<LPR>(widen(vx, vf)));
  if (!live) return;
  kc[row * LPR + sub] = uint2{ekv_fp8_quant4(kf[0], kf[1], kf[2], kf[3], sk), ekv_fp8_quant4(kf[4], kf[5], kf[6], kf[7], sk)};
  vc[row * LPR + sub] = uint2{ekv_fp8_quant4(vf[0], vf[1], vf[2], vf[3], sv), ekv_fp8_quant4(vf[4], vf[5], vf[6], vf[7], sv)};
  if (sub == 0) {
    ks[row] = sk;
    vs[row] = sv;
  }
}

// OUT: 0 fp16, 1 bf16, 2 fp32.  One thread per 8 codes; out is dense [rows][D].
template <int D, int OUT>
__global__ void __launch_bounds__(256) ekv_kv8_dequantize_kernel(const uint2* __restrict__ kc, const uint2* __restrict__ vc, const float* __restrict__ ks,
                                                                 const float* __restrict__ vs, void* __restrict__ k_out, void* __restrict__ v_out,
                                                                 int n_kv_heads, int cap, int layer_begin, int extent, long long n_rows) {
  constexpr int LPR = D / 8;
  const int sub = threadIdx.x % LPR;
  const long long r = (long long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  if (r >= n_rows) return;
  const size_t row = kv8_row(r, n_kv_heads, cap, layer_begin, extent);
  auto one = [&](const uint2* codes, const float* scales, void* out) {
    const uint2 c = codes[row * LPR + sub];
    const float s = scales[row];
    float f[8];
    ekv_fp8_widen4(c.x, f), ekv_fp8_widen4(c.y, f + 4);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] *= s;
    const size_t o = ((size_t)r * LPR + sub) * 8;
    if (OUT == 2) {
      float4* p = reinterpret_cast<float4*>(static_cast<float*>(out) + o);
      p[0] = float4{f[0], f[1], f[2], f[3]};
      p[1] = float4{f[4], f[5], f[6], f[7]};
    } else {
      uint32_t w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (OUT == 1) {
          typedef __bf16 b2 __attribute__((ext_vector_type(2)));
          w[i] = __builtin_bit_cast(uint32_t, b2{(__bf16)f[2 * i], (__bf16)f[2 * i + 1]});
        } else {
          w[i] = __builtin_bit_cast(uint32_t, __floats2half2_rn(f[2 * i], f[2 * i + 1]));
        }
      }
      *reinterpret_cast<uint4*>(static_cast<uint16_t*>(out) + o) = uint4{w[0], w[1], w[2], w[3]};
    }
  };
  one(kc, ks, k_out);
  one(vc, vs, v_out);
}

}  // namespace

hipError_t ekv_launch_kv8_quantize(const ekv_bank* bank, const ekv_kv8* q8, bool src_bf16, int layer_begin, int layer_count, int extent,
                                   hipStream_t s) {
  const int D = bank->head_dim;
  const long long n_rows = (long long)layer_count * bank->n_kv_heads * extent;
  if (n_rows == 0) return hipSuccess;
  const int rows_per_block = 256 / (D / 8);
  const dim3 grid((unsigned)((n_rows + rows_per_block - 1) / rows_per_block));
#define EKV_KV8_Q(DD, BF)                                                                                                        \
  hipLaunchKernelGGL((ekv_kv8_quantize_kernel<DD, BF>), grid, dim3(256), 0, s, static_cast<const uint4*>(bank->k),              \
                     static_cast<const uint4*>(bank->v), static_cast<uint2*>(q8->k_codes), static_cast<uint2*>(q8->v_codes),    \
                     q8->k_scale, q8->v_scale, bank->n_kv_heads, bank->cap, layer_begin, extent, n_rows)
  if (D == 128) {
    if (src_bf16) EKV_KV8_Q(128, true); else EKV_KV8_Q(128, false);
  } else if (D == 64) {
    if (src_bf16) EKV_KV8_Q(64, true); else EKV_KV8_Q(64, false);
  } else {
    return hipErrorInvalidValue;
  }
#undef EKV_KV8_Q
  return hipGetLastError();
}

hipError_t ekv_launch_kv8_dequantize(const ekv_bank* bank, const ekv_kv8* q8, int out_kind, int layer_begin, int layer_count, int extent,
                                     void* k_out, void* v_out, hipStream_t s) {
  const int D = bank->head_dim;
  const long long n_rows = (long long)layer_count * bank->n_kv_heads * extent;
  if (n_rows == 0) return hipSuccess;
  const int rows_per_block = 256 / (D / 8);
  const dim3 grid((unsigned)((n_rows + rows_per_block - 1) / rows_per_block));
#define EKV_KV8_DQ(DD, OUT)                                                                                                      \
  hipLaunchKernelGGL((ekv_kv8_dequantize_kernel<DD, OUT>), grid, dim3(256), 0, s, static_cast<const uint2*>(q8->k_codes),       \
                     static_cast<const uint2*>(q8->v_codes), q8->k_scale, q8->v_scale, k_out, v_out, bank->n_kv_heads, bank->cap, \
                     layer_begin, extent, n_rows)
  if (D != 64 && D != 128) return hipErrorInvalidValue;
  switch (out_kind) {
    case 0: if (D == 128) EKV_KV8_DQ(128, 0); else EKV_KV8_DQ(64, 0); break;
    case 1: if (D == 128) EKV_KV8_DQ(128, 1); else EKV_KV8_DQ(64, 1); break;
    case 2: if (D == 128) EKV_KV8_DQ(128, 2); else EKV_KV8_DQ(64, 2); break;
    default: return hipErrorInvalidValue;
  }
#undef EKV_KV8_DQ
  return hipGetLastError();
}
