// ekv_softcap_eval (include/easykv_hip.h): out[i] = ekv_softcap(x[i] / sm_div, cap) — the inline every EKV_SOFTCAP kernel calls, on its
// own, for tests and tooling.  One object (the EKV_SOFTCAP_EVAL line of ekv_instances_later.def).
#include "ekv_common.h"
#include "ekv_kernels.h"

namespace {
__global__ void __launch_bounds__(EKV_EVAL_NT) ekv_softcap_eval_kernel(const float* x, int64_t n, float sm_div, float cap, float* out) {
  const int64_t i = (int64_t)blockIdx.x * EKV_EVAL_NT + threadIdx.x;
  if (i < n) out[i] = ekv_softcap(x[i] / sm_div, cap);
}
}  // namespace

hipError_t ekv_launch_softcap_eval(const float* x, int64_t n, float sm_div, float cap, float* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + EKV_EVAL_NT - 1) / EKV_EVAL_NT;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ekv_softcap_eval_kernel, dim3((unsigned)blocks), dim3(EKV_EVAL_NT), 0, s, x, n, sm_div, cap, out);
  return hipGetLastError();
}
