// Launch code of the MFMA decode kernel for MXFP4 rows (ekv_attn_decode_mxg.inc; which steps run there: resolve_call, ekv_plan.cpp, "grouped").
#include "ekv_common.h"
#include "ekv_kernels.h"

// ---- the instances (the EKV_DECODE_MXG lines of the manifest): launcher declarations, then one table entry per line
typedef hipError_t EkvDecodeMxgFn(const EkvAttnArgs&, int layer_count, hipStream_t);
#define EKV_DECODE_MXG(elem, d) EkvDecodeMxgFn EKV_FN_D_ELEM(ekv_launch_attn_decode_mxg, d, elem);
#include "ekv_instances.def"

namespace {
struct DecodeMxgInstance {
  int head_dim;
  bool bf16;
  EkvDecodeMxgFn* fn;
};
const DecodeMxgInstance kDecodeMxg[] = {
#define EKV_DECODE_MXG(elem, d) {d, EKV_IS_##elem, EKV_FN_D_ELEM(ekv_launch_attn_decode_mxg, d, elem)},
#include "ekv_instances.def"
};
}  // namespace

hipError_t ekv_launch_attn_decode_mxg(const EkvAttnArgs& a, int head_dim, int layer_count, hipStream_t s, bool bf16) {
  for (const DecodeMxgInstance& in : kDecodeMxg)
    if (in.head_dim == head_dim && in.bf16 == bf16) return in.fn(a, layer_count, s);
  return hipErrorInvalidValue;
}
