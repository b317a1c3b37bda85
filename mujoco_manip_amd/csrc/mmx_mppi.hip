// The MPPI planner's own kernels (mmx_mppi_plan, include/mmx_api.h): sample the candidates before the
// rollout, reweight after it.  The closed forms are mmx_mppi.h's (shared with the host self-test).
//
//   mmx_mppi_sample_kernel   one thread per (planner env i, component a), a loop over the horizon: xi (the
//                            caller's, or Philox4x32-10 + Box-Muller) -> beta filter -> noise, actions.  Threads
//                            are consecutive along [i][a], so every step's stores are coalesced.
//   mmx_mppi_update_kernel   one workgroup of kWG threads per controlled env: returns of candidates
//                            k = tid, tid + kWG, ..., the group's max (lowest k on ties) and weight sum, the
//                            weights, then the H x A weighted sums, the shift and the output action.
//   mmx_mppi_fill_kernel     mmx_mppi_reset: one action row to every step of the nominal plans.
//
// Every reduction has a fixed order: a lane's strided partial, a DPP butterfly within each row of 16 lanes
// (both partners combine the same two values, so every lane of the row holds the same bits), the wave's
// four rows in row order, the waves' results through LDS in wave order.  No atomics.  The accumulators are
// indexed by unrolled constants only (registers, no scratch).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mmx_launch.h"
#include "mmx_mppi.h"

namespace {

constexpr int kWG = 256, kWaves = kWG / 64;

// the value of the lane that CTRL names within the row of 16 lanes (every control used here names an
// active lane: all 64 lanes take part in every reduction)
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(dpp_i<CTRL>(__float_as_int(v)));
}
constexpr int kQuadSwap1 = 0xB1, kQuadSwap2 = 0x4E, kHalfMirror = 0x141, kRowMirror = 0x140;  // quad_perm [1,0,3,2], [2,3,0,1]

// the wave's sum in every lane: a butterfly within each row of 16 lanes, then the four rows in row order
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_f<kQuadSwap1>(v);
  v += dpp_f<kQuadSwap2>(v);
  v += dpp_f<kHalfMirror>(v);
  v += dpp_f<kRowMirror>(v);
  const int b = __float_as_int(v);
  return ((__int_as_float(__builtin_amdgcn_readlane(b, 0)) + __int_as_float(__builtin_amdgcn_readlane(b, 16))) +
          __int_as_float(__builtin_amdgcn_readlane(b, 32))) + __int_as_float(__builtin_amdgcn_readlane(b, 48));
}
// the wave's best (return, candidate) in every lane, the same way
template <int CTRL>
__device__ __forceinline__ void best_step(float& bv, int& bk) {
  const float ov = dpp_f<CTRL>(bv);
  const int ok = dpp_i<CTRL>(bk);
  if (mppi_better(ov, ok, bv, bk)) bv = ov, bk = ok;
}
__device__ __forceinline__ void wave_best(float& bv, int& bk) {
  best_step<kQuadSwap1>(bv, bk);
  best_step<kQuadSwap2>(bv, bk);
  best_step<kHalfMirror>(bv, bk);
  best_step<kRowMirror>(bv, bk);
  const int vb = __float_as_int(bv), kb = bk;
  bv = __int_as_float(__builtin_amdgcn_readlane(vb, 0));
  bk = __builtin_amdgcn_readlane(kb, 0);
#pragma unroll
  for (int row = 1; row < 4; row++) {
    const float ov = __int_as_float(__builtin_amdgcn_readlane(vb, 16 * row));
    const int ok = __builtin_amdgcn_readlane(kb, 16 * row);
    if (mppi_better(ov, ok, bv, bk)) bv = ov, bk = ok;
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(kWG)
mmx_mppi_sample_kernel(MppiParams P, MppiBufs B, const float* box, const float* xi) {
  const size_t A = (size_t)P.A, K = (size_t)P.K, M = (size_t)P.M, NA = M * K * A;
  const size_t idx = (size_t)blockIdx.x * kWG + threadIdx.x;
  if (idx >= NA) return;
  const size_t i = idx / A, a = idx - i * A, m = i / K;
  const bool nominal_row = i - m * K == 0;  // candidate 0 of the group: the nominal plan itself
  const float sigma = box[a], lo = box[MPPI_MAX_ADIM + a], hi = box[2 * MPPI_MAX_ADIM + a];
  float eps = 0.f;
  for (int t = 0; t < P.H; t++) {
    const size_t e = (size_t)t * NA + idx;
    const float x = xi ? xi[e] : mppi_draw(P.seed_lo, P.seed_hi, P.call_lo, P.call_hi, (uint32_t)t, (uint32_t)i, (uint32_t)a);
    eps = t == 0 ? x : mppi_filter(P.beta, P.beta_c, eps, x);
    const float n = nominal_row ? 0.f : eps;
    B.noise[e] = n;
    B.actions[e] = mppi_action(B.nominal[((size_t)t * M + m) * A + a], sigma, n, lo, hi);
  }
}

extern "C" __global__ void __launch_bounds__(kWG)
mmx_mppi_update_kernel(MppiParams P, MppiBufs B, const float* box, float* action_out) {
  __shared__ float s_val[kWaves];
  __shared__ int s_idx[kWaves];
  __shared__ float s_sum[kWaves];
  __shared__ float s_part[MPPI_MAX_HORIZON][kWaves][MPPI_MAX_ADIM];
  __shared__ float s_new[MPPI_MAX_HORIZON * MPPI_MAX_ADIM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t A = (size_t)P.A, K = (size_t)P.K, M = (size_t)P.M, N = M * K, m = blockIdx.x, i0 = m * K;
  const int HA = P.H * P.A;

  // returns, and the group's maximum over the finite ones
  float bv = 0.f;
  int bk = -1;
  for (size_t k = tid; k < K; k += kWG) {
    const float R = mppi_return(B.reward, B.done, N, i0 + k, P.H, P.gamma);
    B.returns[i0 + k] = R;
    if (mppi_finite(R) && mppi_better(R, (int)k, bv, bk)) bv = R, bk = (int)k;
  }
  wave_best(bv, bk);
  if (lane == 0) s_val[wave] = bv, s_idx[wave] = bk;
  __syncthreads();
  bv = s_val[0], bk = s_idx[0];
#pragma unroll
  for (int w = 1; w < kWaves; w++)
    if (mppi_better(s_val[w], s_idx[w], bv, bk)) bv = s_val[w], bk = s_idx[w];
  if (tid == 0) B.best[m] = bk;
  if (bk < 0) {  // the whole group is excluded (uniform over the workgroup): weights 0, the nominal kept
    for (size_t k = tid; k < K; k += kWG) B.weights[i0 + k] = 0.f;
    if (tid < P.A) action_out[m * A + tid] = B.nominal[m * A + tid];
    return;
  }

  // weights: every thread reads back only the entries it wrote itself
  float part = 0.f;
  for (size_t k = tid; k < K; k += kWG) {
    const float R = B.returns[i0 + k];
    float e = 0.f;
    if (mppi_finite(R)) e = P.inv_lambda > 0.f ? mppi_weight(R, bv, P.inv_lambda) : ((int)k == bk ? 1.f : 0.f);
    B.weights[i0 + k] = e;
    part += e;
  }
  part = wave_sum(part);
  if (lane == 0) s_sum[wave] = part;
  __syncthreads();
  float total = s_sum[0];
#pragma unroll
  for (int w = 1; w < kWaves; w++) total += s_sum[w];
  const float inv = 1.f / total;  // total >= 1: the best candidate's weight is exp(0)
  for (size_t k = tid; k < K; k += kWG) B.weights[i0 + k] *= inv;

  // nominal'[t][a] = sum_k w_k actions[t][i0 + k][a]
  for (int t = 0; t < P.H; t++) {
    float acc[MPPI_MAX_ADIM];
#pragma unroll
    for (int a = 0; a < MPPI_MAX_ADIM; a++) acc[a] = 0.f;
    for (size_t k = tid; k < K; k += kWG) {
      const float w = B.weights[i0 + k];
      const float* row = B.actions + ((size_t)t * N + i0 + k) * A;
#pragma unroll
      for (int a = 0; a < MPPI_MAX_ADIM; a++)
        if (a < P.A) acc[a] = fmaf(w, row[a], acc[a]);
    }
#pragma unroll
    for (int a = 0; a < MPPI_MAX_ADIM; a++)
      if (a < P.A) {
        const float v = wave_sum(acc[a]);
        if (lane == 0) s_part[t][wave][a] = v;
      }
  }
  __syncthreads();
  for (int j = tid; j < HA; j += kWG) {
    const int t = j / P.A, a = j - t * P.A;
    float v = s_part[t][0][a];
#pragma unroll
    for (int w = 1; w < kWaves; w++) v += s_part[t][w][a];
    // (a convex combination of clamped actions: the clamp only removes a last-bit excess of the sum)
    s_new[j] = mppi_clamp(v, box[MPPI_MAX_ADIM + a], box[2 * MPPI_MAX_ADIM + a]);
  }
  __syncthreads();
  // the output, and the shift: step t of the next call's nominal is step t + 1 of this one, the last repeated
  for (int j = tid; j < HA; j += kWG) {
    const int t = j / P.A, a = j - t * P.A;
    const int from = t + 1 < P.H ? t + 1 : t;
    B.nominal[((size_t)t * M + m) * A + a] = s_new[from * P.A + a];
    if (t == 0) action_out[m * A + a] = s_new[a];
  }
}

extern "C" __global__ void __launch_bounds__(kWG)
mmx_mppi_fill_kernel(MppiParams P, float* nominal, const float* box, const float* action) {
  const size_t MA = (size_t)P.M * P.A, n = (size_t)P.H * MA;
  const size_t idx = (size_t)blockIdx.x * kWG + threadIdx.x;
  if (idx >= n) return;
  const size_t r = idx % MA, a = r % (size_t)P.A;
  nominal[idx] = mppi_clamp(action[r], box[MPPI_MAX_ADIM + a], box[2 * MPPI_MAX_ADIM + a]);
}

extern "C" hipError_t mmx_launch_mppi_sample(const MppiParams* P, const MppiBufs* B, const float* box, const float* xi,
                                             hipStream_t st) {
  const size_t n = (size_t)P->M * P->K * P->A;
  hipLaunchKernelGGL(mmx_mppi_sample_kernel, dim3((unsigned)((n + kWG - 1) / kWG)), dim3(kWG), 0, st, *P, *B, box, xi);
  return hipGetLastError();
}
extern "C" hipError_t mmx_launch_mppi_update(const MppiParams* P, const MppiBufs* B, const float* box, float* action_out,
                                             hipStream_t st) {
  hipLaunchKernelGGL(mmx_mppi_update_kernel, dim3((unsigned)P->M), dim3(kWG), 0, st, *P, *B, box, action_out);
  return hipGetLastError();
}
extern "C" hipError_t mmx_launch_mppi_fill(const MppiParams* P, float* nominal, const float* box, const float* action,
                                           hipStream_t st) {
  const size_t n = (size_t)P->H * P->M * P->A;
  hipLaunchKernelGGL(mmx_mppi_fill_kernel, dim3((unsigned)((n + kWG - 1) / kWG)), dim3(kWG), 0, st, *P, nominal, box, action);
  return hipGetLastError();
}
