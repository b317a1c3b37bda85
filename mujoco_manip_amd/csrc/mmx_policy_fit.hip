// The MLP policy's training step (mmx_policy_fit, include/mmx_api.h; the closed forms: mmx_policy_fit.h): one
// optimisation step is three launches on the policy's stream, and the host loops them without synchronising.
//
//   mmx_fit_forward_kernel   one workgroup per tile of FIT_TS samples: gathers the tile's observations by index,
//                            normalises them into LDS, runs the layers forward (thread j = neuron j with one
//                            accumulator per sample: policy_neuron's chain, a weight read once per tile), saves every
//                            layer's input to the workspace, forms the output delta and the tile's loss partial, and
//                            runs the deltas backward through W^T and act' (thread k = unit k), saving them.
//   mmx_fit_wgrad_kernel     per layer the GEMM X^T D ([in + 1 x B] . [B x out]; row `in` of X^T is the constant 1
//                            whose weight is the bias) on the fp32 matrix cores, v_mfma_f32_16x16x4_f32: a
//                            workgroup of four waves owns a 64 x 64 tile of the layer's gradient over one chunk of
//                            FIT_KC samples (blockIdx.y), each wave a 32 x 32 quarter = four independent
//                            accumulators; the operands are staged through LDS 32 samples (kKS) at a time, padded
//                            with zeros past the batch, the layer and the chunk.  Every chunk's partial is written
//                            out, laid out like the blob.  The MFMA is a k-ordered fmaf chain, so a partial is the
//                            chunk's samples summed in index order.  The thin last layer (out = A <= 10) takes the
//                            same path: one 64-wide column tile, its padding columns multiplied as zeros.
//   mmx_fit_update_kernel    one lane per real parameter (j < out): the chunk partials summed in chunk order, the
//                            optimiser, the weight written into the blob in place (m and v into their arrays); one
//                            more workgroup sums the tiles' loss partials in tile order into loss_out[k].
//
// No atomics; every sum's order is fixed by (B, the layer sizes) alone.  The workspace (float offsets, B = batch):
//   x_l [B][in_l] for l = 0 .. L-1, then d_l [B][out_l], then the loss partials [ceil(B / FIT_TS)], then the chunk
//   partials [ceil(B / FIT_KC)][policy_fit_param_floats], then the PG statistics' partials [ceil(B / FIT_TS)][3].
//
// The policy-gradient step (mmx_policy_fit_pg; the closed forms: mmx_pg.h) is the same step with another output
// delta, four launches:
//   mmx_pg_forward_kernel    the pass above (one text, mmx_fit_forward.inc) with PPO's clipped surrogate: the A output
//                            threads exchange z and z' through LDS, each forms the samples' ratios and its own delta,
//                            thread 0 the tile's three statistic partials
//   mmx_fit_wgrad_kernel, mmx_fit_update_kernel    as they are (no loss_out)
//   mmx_pg_stats_kernel      one workgroup: the tiles' partials in tile order into stats_out[k][3]
// and, for mmx_gae: mmx_gae_kernel (one lane per env column, t backward: rows [t][N] read and written coalesced),
// mmx_pg_moments_kernel (one workgroup of PG_SUM_LANES threads: both sums in pg_sum's shape) and
// mmx_pg_rescale_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mmx_launch.h"
#include "mmx_pg.h"
#include "mmx_policy_fit.h"

namespace {
constexpr int kTS = FIT_TS, kThreads = 256;
constexpr int kKS = 32;          // samples staged per LDS block of the GEMM
constexpr int kStride = 64 + 16; // LDS row of a staged block: the four rows a ds_read_b32 of the MFMA operands touches
                                 // per 32-lane half fall on disjoint halves of the 32 banks (80 mod 32 = 16)
typedef __attribute__((ext_vector_type(4))) float f32x4;

// the layer's input offset (floats) in the workspace: B * (in_0 + .. + in_{l-1}); fields read one by one (scalar)
__device__ __forceinline__ size_t fit_x_off(const MmxPolicy& P, int l, int B) {
  size_t w = 0;
  for (int i = 0; i < l; i++) w += (size_t)policy_u(P.in[i]);
  return w * (size_t)B;
}
__device__ __forceinline__ size_t fit_d_off(const MmxPolicy& P, int l, int B) {
  size_t w = 0;
  for (int i = 0; i < l; i++) w += (size_t)policy_u(P.out[i]);
  return w * (size_t)B;
}
}  // namespace

// ------------------------------------------------------------------ forward pass and deltas
#define FIT_PG 0
#include "mmx_fit_forward.inc"
#undef FIT_PG
#define FIT_PG 1
#include "mmx_fit_forward.inc"
#undef FIT_PG

// ------------------------------------------------------------------ weight gradients: X^T D per layer and K chunk
extern "C" __global__ void __launch_bounds__(kThreads)
mmx_fit_wgrad_kernel(MmxPolicy P, MmxFit F) {
  __shared__ float Xs[kKS * kStride], Ds[kKS * kStride];
  const int l = (int)blockIdx.z;
  const int in = policy_u(P.in[l]), out = policy_u(P.out[l]), outp = policy_padded(out), B = F.B;
  const int tiles_n = outp / 64, tiles_m = (in + 1 + 63) / 64;
  const int tm = (int)blockIdx.x / tiles_n, tn = (int)blockIdx.x - tm * tiles_n;
  if (tm >= tiles_m) return;  // the grid is sized for the largest layer
  const int tid = threadIdx.x, lane = tid & 63, wave = policy_u(tid >> 6);
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int s_begin = (int)blockIdx.y * FIT_KC, s_end = min(B, s_begin + FIT_KC);
  const float* X = F.ws + fit_x_off(P, l, B);
  const float* D = F.ws + F.d_base + fit_d_off(P, l, B);

  f32x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int c = tid & 63, r0 = tid >> 6;  // this thread's column of a staged block, and its first row (then + 4)
  const int mcol = tm * 64 + c, ncol = tn * 64 + c;
  for (int sb = s_begin; sb < s_end; sb += kKS) {
#pragma unroll
    for (int r = r0; r < kKS; r += kThreads / 64) {
      const int s = sb + r;
      float xv = 0.f, dv = 0.f;
      if (s < s_end) {
        xv = mcol < in ? X[(size_t)s * (size_t)in + (size_t)mcol] : (mcol == in ? 1.f : 0.f);
        if (ncol < out) dv = D[(size_t)s * (size_t)out + (size_t)ncol];
      }
      Xs[r * kStride + c] = xv;
      Ds[r * kStride + c] = dv;
    }
    __syncthreads();
    // lane: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]
    const float* xa = Xs + (lane >> 4) * kStride + wm + (lane & 15);
    const float* db = Ds + (lane >> 4) * kStride + wn + (lane & 15);
#pragma unroll
    for (int kk = 0; kk < kKS / 4; kk++) {
      const float a0 = xa[kk * 4 * kStride], a1 = xa[kk * 4 * kStride + 16];
      const float b0 = db[kk * 4 * kStride], b1 = db[kk * 4 * kStride + 16];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  // C: column = lane & 15, row = 4 (lane >> 4) + register
  float* part = F.ws + F.part_base + (size_t)blockIdx.y * (size_t)policy_u(P.shift_off) + (size_t)policy_u(P.woff[l]);
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int m = tm * 64 + wm + a * 16 + 4 * (lane >> 4) + r, j = tn * 64 + wn + b * 16 + (lane & 15);
        if (m <= in && j < out) part[(size_t)m * (size_t)outp + (size_t)j] = acc[a][b][r];
      }
}

// ------------------------------------------------------------------ reduce the partials, apply the optimiser
extern "C" __global__ void __launch_bounds__(kThreads)
mmx_fit_update_kernel(MmxPolicy P, MmxFit F, MmxFitOpt O, float* blob, float* m, float* v, float* loss_out) {
  const int total = policy_u(P.shift_off);
  const int blocks = (total + kThreads - 1) / kThreads;
  if ((int)blockIdx.x == blocks) {  // the loss: the tiles' partials in tile order
    if (threadIdx.x == 0 && loss_out) {
      const int tiles = (F.B + kTS - 1) / kTS;
      const float* lp = F.ws + F.loss_base;
      float acc = 0.f;
      for (int t = 0; t < tiles; t++) acc += lp[t];
      *loss_out = acc * F.inv_count;
    }
    return;
  }
  const int e = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (e >= total) return;
  // the lane's layer, by constant indices (a lane-indexed read of P's arrays would put them in scratch memory)
  const int L = policy_u(P.n_layers);
  int woff = 0, out = policy_u(P.out[0]);
#pragma unroll
  for (int i = 1; i < POLICY_MAX_LAYERS; i++)
    if (i < L && e >= policy_u(P.woff[i])) woff = policy_u(P.woff[i]), out = policy_u(P.out[i]);
  const int j = (e - woff) % policy_padded(out);
  if (j >= out) return;  // a padding column: never written, stays 0
  const int chunks = (F.B + FIT_KC - 1) / FIT_KC;
  const float* part = F.ws + F.part_base + (size_t)e;
  float g = part[0];
  for (int ch = 1; ch < chunks; ch++) g += part[(size_t)ch * (size_t)total];
  float mv = 0.f, vv = 0.f;
  if (O.optimizer == FIT_ADAM) mv = m[e], vv = v[e];
  blob[e] = policy_fit_update(blob[e], g, &mv, &vv, O);
  if (O.optimizer == FIT_ADAM) m[e] = mv, v[e] = vv;
}

extern "C" size_t mmx_policy_fit_workspace_floats(const MmxPolicy* P, int B, MmxFit* F) {
  size_t xw = 0, dw = 0;
  for (int l = 0; l < P->n_layers; l++) xw += (size_t)P->in[l], dw += (size_t)P->out[l];
  const size_t tiles = ((size_t)B + kTS - 1) / kTS, chunks = ((size_t)B + FIT_KC - 1) / FIT_KC;
  const size_t d_base = xw * (size_t)B, loss_base = d_base + dw * (size_t)B, part_base = (loss_base + tiles + 63) / 64 * 64;
  if (F) F->d_base = d_base, F->loss_base = loss_base, F->part_base = part_base;
  return part_base + chunks * policy_fit_param_floats(*P);
}

extern "C" hipError_t mmx_launch_policy_fit_step(const MmxPolicy* P, const MmxFit* F, const MmxFitOpt* O, float* blob, float* m,
                                                 float* v, float* loss_out, hipStream_t st) {
  const int B = F->B, tiles = (B + kTS - 1) / kTS, chunks = (B + FIT_KC - 1) / FIT_KC;
  int wtiles = 1;
  for (int l = 0; l < P->n_layers; l++) wtiles = std::max(wtiles, (P->in[l] + 1 + 63) / 64 * (policy_padded(P->out[l]) / 64));
  const int ublocks = (P->shift_off + kThreads - 1) / kThreads + 1;
  hipLaunchKernelGGL(mmx_fit_forward_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, *P, *F);
  hipLaunchKernelGGL(mmx_fit_wgrad_kernel, dim3((unsigned)wtiles, (unsigned)chunks, (unsigned)P->n_layers), dim3(kThreads), 0, st, *P, *F);
  hipLaunchKernelGGL(mmx_fit_update_kernel, dim3((unsigned)ublocks), dim3(kThreads), 0, st, *P, *F, *O, blob, m, v, loss_out);
  return hipGetLastError();
}

// ------------------------------------------------------------------ the policy-gradient step's own launches
extern "C" __global__ void __launch_bounds__(64)
mmx_pg_stats_kernel(MmxFit F, MmxPg G, float* stats_out) {
#pragma clang fp contract(off)
  const int c = threadIdx.x;  // lane c sums statistic c, the tiles in order
  if (c >= 3) return;
  const int tiles = (F.B + kTS - 1) / kTS;
  const float* sp = F.ws + G.stat_base + c;
  float acc = 0.f;
  for (int t = 0; t < tiles; t++) acc += sp[(size_t)t * 3];
  stats_out[c] = acc * G.invB;
}

extern "C" size_t mmx_policy_fit_pg_workspace_floats(const MmxPolicy* P, int B, MmxFit* F, MmxPg* G) {
  const size_t stat_base = (mmx_policy_fit_workspace_floats(P, B, F) + 63) / 64 * 64;
  if (G) G->stat_base = stat_base;
  return stat_base + 3 * (((size_t)B + kTS - 1) / kTS);
}

extern "C" hipError_t mmx_launch_policy_fit_pg_step(const MmxPolicy* P, const MmxFit* F, const MmxPg* G, const MmxFitOpt* O, float* blob,
                                                    float* m, float* v, float* stats_out, hipStream_t st) {
  const int B = F->B, tiles = (B + kTS - 1) / kTS, chunks = (B + FIT_KC - 1) / FIT_KC;
  int wtiles = 1;
  for (int l = 0; l < P->n_layers; l++) wtiles = std::max(wtiles, (P->in[l] + 1 + 63) / 64 * (policy_padded(P->out[l]) / 64));
  const int ublocks = (P->shift_off + kThreads - 1) / kThreads + 1;
  hipLaunchKernelGGL(mmx_pg_forward_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, *P, *F, *G);
  hipLaunchKernelGGL(mmx_fit_wgrad_kernel, dim3((unsigned)wtiles, (unsigned)chunks, (unsigned)P->n_layers), dim3(kThreads), 0, st, *P, *F);
  hipLaunchKernelGGL(mmx_fit_update_kernel, dim3((unsigned)ublocks), dim3(kThreads), 0, st, *P, *F, *O, blob, m, v, (float*)nullptr);
  if (stats_out) hipLaunchKernelGGL(mmx_pg_stats_kernel, dim3(1), dim3(64), 0, st, *F, *G, stats_out);
  return hipGetLastError();
}

// ------------------------------------------------------------------ GAE and the advantages' normalisation
extern "C" __global__ void __launch_bounds__(kThreads)
mmx_gae_kernel(float gamma, float gl, int T, int N, const float* __restrict__ reward, const int32_t* __restrict__ done,
               const float* __restrict__ value, const float* __restrict__ value_last, float* __restrict__ adv_out,
               float* __restrict__ ret_out) {
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;  // the env column
  if (i >= N) return;
  float adv = 0.f, nv = value_last[i];
  for (int t = T - 1; t >= 0; t--) {
    const size_t e = (size_t)t * (size_t)N + (size_t)i;
    const float val = value[e];
    float ret;
    adv = pg_gae_step(gamma, gl, done[3 * e], done[3 * e + 1], reward[e], val, nv, adv, &ret);
    adv_out[e] = adv;
    if (ret_out) ret_out[e] = ret;
    nv = val;  // value[t] is step t - 1's next value
  }
}

// one workgroup: moments[0] = the mean, moments[1] = sqrtf(var) + 1e-8f; the sums in pg_sum's shape (mmx_pg.h)
extern "C" __global__ void __launch_bounds__(PG_SUM_LANES)
mmx_pg_moments_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ moments) {
#pragma clang fp contract(off)
  __shared__ float chain[PG_SUM_LANES];
  const int tid = threadIdx.x;
  const float nf = (float)n;
  float mean = 0.f;
  for (int square = 0; square < 2; square++) {
    float acc = 0.f;
    for (int64_t e = tid; e < n; e += PG_SUM_LANES) acc += pg_sum_term(x[e], mean, square);
    chain[tid] = acc;
    __syncthreads();
    for (int stride = PG_SUM_LANES / 2; stride >= 1; stride >>= 1) {
      if (tid < stride) chain[tid] += chain[tid + stride];
      __syncthreads();
    }
    const float sum = chain[0];
    __syncthreads();  // chain is written again by the second pass
    if (!square) mean = sum / nf;
    else if (tid == 0) moments[0] = mean, moments[1] = pg_norm_denominator(sum, nf);
  }
}
extern "C" __global__ void __launch_bounds__(kThreads)
mmx_pg_rescale_kernel(float* __restrict__ x, int64_t n, const float* __restrict__ moments) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + (int64_t)threadIdx.x;
  if (e < n) x[e] = pg_normalise(x[e], moments[0], moments[1]);
}

extern "C" hipError_t mmx_launch_gae(float gamma, float gl, int T, int N, const float* reward, const int32_t* done, const float* value,
                                     const float* value_last, float* adv_out, float* ret_out, float* moments, hipStream_t st) {
  hipLaunchKernelGGL(mmx_gae_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, gamma, gl, T, N, reward, done,
                     value, value_last, adv_out, ret_out);
  if (moments) {  // normalise
    const int64_t n = (int64_t)T * (int64_t)N;
    hipLaunchKernelGGL(mmx_pg_moments_kernel, dim3(1), dim3(PG_SUM_LANES), 0, st, (const float*)adv_out, n, moments);
    hipLaunchKernelGGL(mmx_pg_rescale_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, adv_out, n,
                       (const float*)moments);
  }
  return hipGetLastError();
}
