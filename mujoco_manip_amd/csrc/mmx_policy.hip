// The MLP policy's network alone (mmx_policy_eval, include/mmx_api.h): observations the caller supplies ->
// the network's output (the mean, before noise and clamp).  One wave per row: the forward pass is
// policy_forward_wave of mmx_policy.h, the very function mmx_env_policy_kernel (mmx_step_kernels.inc) runs between two env
// steps, here on LDS of its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mmx_launch.h"
#include "mmx_policy.h"

namespace {
constexpr int kIn = (POLICY_NOBS + 3) & ~3;  // the input's slot, then the two activation buffers
}

extern "C" __global__ void __launch_bounds__(POLICY_LANES)
mmx_policy_eval_kernel(MmxPolicy P, const float* obs, int n, float* mean_out) {
  __shared__ float s[kIn + 2 * POLICY_MAX_WIDTH];
  const size_t row = blockIdx.x;
  if (row >= (size_t)n) return;
  const int lane = threadIdx.x;
  const float* data = policy_data(P);
  for (int k = lane; k < POLICY_NOBS; k += POLICY_LANES)
    s[k] = policy_normalise(obs[row * POLICY_NOBS + k], data[P.shift_off + k], data[P.scale_off + k]);
  policy_wave_sync();
  const float* out = policy_forward_wave(P, data, s, s + kIn, s + kIn + POLICY_MAX_WIDTH, lane);
  if (lane < P.A) mean_out[row * (size_t)P.A + lane] = out[lane];
}

extern "C" hipError_t mmx_launch_policy_eval(const MmxPolicy* P, const float* obs, int n, float* mean_out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(mmx_policy_eval_kernel, dim3((unsigned)n), dim3(POLICY_LANES), 0, st, *P, obs, n, mean_out);
  return hipGetLastError();
}
