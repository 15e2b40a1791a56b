// Launch code of the MFMA decode kernel for FP8 rows (ekv_attn_decode_g8.inc; which steps run there: resolve_call, ekv_plan.cpp, "grouped").
#include "ekv_common.h"
#include "ekv_kernels.h"

// ---- the instances (the EKV_DECODE_G8 lines of the manifest): launcher declarations, then one table entry per line
typedef hipError_t EkvDecodeG8Fn(const EkvAttnArgs&, int layer_count, hipStream_t);
#define EKV_DECODE_G8(elem, d) EkvDecodeG8Fn EKV_FN_D_ELEM(ekv_launch_attn_decode_g8, d, elem);
#include "ekv_instances.def"

namespace {
struct DecodeG8Instance {
  int head_dim;
  bool bf16;
  EkvDecodeG8Fn* fn;
};
const DecodeG8Instance kDecodeG8[] = {
#define EKV_DECODE_G8(elem, d) {d, EKV_IS_##elem, EKV_FN_D_ELEM(ekv_launch_attn_decode_g8, d, elem)},
#include "ekv_instances.def"
};
}  // namespace

hipError_t ekv_launch_attn_decode_g8(const EkvAttnArgs& a, int head_dim, int layer_count, hipStream_t s, bool bf16) {
  for (const DecodeG8Instance& in : kDecodeG8)
    if (in.head_dim == head_dim && in.bf16 == bf16) return in.fn(a, layer_count, s);
  return hipErrorInvalidValue;
}
