// The closed forms of the MLP policy (mmx_policy_create / mmx_policy_eval / mmx_rollout_policy, include/mmx_api.h)
// as host + device inline functions: mmx_env_policy_kernel (mmx_step_kernels.inc) and mmx_policy_eval_kernel
// (mmx_policy.hip) call them, and a stand-alone host program (tests/host/mmx_policy_selftest.cpp, plain g++) runs
// the very same code.  The packed-weight indexing, one neuron's dot product, the activation, the action formula, a
// scalar reference of the whole forward pass, and the wave's forward pass over LDS scratch.
//
// The device blob (floats; built once by policy_pack on the host at mmx_policy_create):
//   layer l   weights transposed to [in_l][outp_l], outp_l = out_l rounded up to 64 (the padding columns are 0), so
//             lane j's read of neuron j + 64 q for input k is one coalesced row read; then the bias [outp_l]
//             (a NULL bias and the padding are 0).  in_0 = 85 (the numeric observation), in_l = out_{l-1}.
//   then      obs_shift [85], obs_scale [85], std [POLICY_MAX_ADIM] = exp(log_std), low, high [POLICY_MAX_ADIM].
// The noise of element (rollout step t, env i, component a) is mppi_draw(seed, call, t, i, a) of mmx_mppi.h.
#ifndef MMX_POLICY_H
#define MMX_POLICY_H
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mmx_mppi.h"

#define POLICY_HD MPPI_HD
#define POLICY_MAX_LAYERS 4   // MMX_POLICY_MAX_LAYERS
#define POLICY_MAX_WIDTH 256  // MMX_POLICY_MAX_WIDTH
#define POLICY_MAX_ADIM MPPI_MAX_ADIM
#define POLICY_NOBS 85        // MMX_NOBS: the network's input
#define POLICY_TANH 0         // MMX_POLICY_TANH
#define POLICY_RELU 1         // MMX_POLICY_RELU
#define POLICY_LANES 64

// What a launch needs of a policy (by value: kernel arguments); offsets are in floats into `data`
struct MmxPolicy {
  int n_layers, activation, A, stochastic;
  int in[POLICY_MAX_LAYERS], out[POLICY_MAX_LAYERS];
  int woff[POLICY_MAX_LAYERS], boff[POLICY_MAX_LAYERS];
  int shift_off, scale_off, std_off, low_off, high_off;
  uint32_t seed_lo, seed_hi, call_lo, call_hi;
  const float* data;  // device
};
// The policy's own record of a rollout: device arrays [T][N][A]; actions is the hand-off to the step, the other
// two may be null
struct MMXPolicyRec {
  float* actions;
  float* mean;
  float* noise;
};

// ---- packed-weight indexing
POLICY_HD int policy_padded(int out) { return (out + POLICY_LANES - 1) / POLICY_LANES * POLICY_LANES; }
// weight (neuron j, input k) of a layer with `out` neurons, relative to the layer's woff; j < policy_padded(out)
POLICY_HD size_t policy_windex(int out, int k, int j) { return (size_t)k * (size_t)policy_padded(out) + (size_t)j; }
// floats of one layer (weights, then bias) and of the whole blob
POLICY_HD size_t policy_layer_floats(int in, int out) { return ((size_t)in + 1) * (size_t)policy_padded(out); }
// fills the offsets of P from n_layers / in / out; returns the blob's size in floats
inline size_t policy_layout(MmxPolicy& P) {
  size_t at = 0;
  for (int l = 0; l < P.n_layers; l++) {
    P.woff[l] = (int)at;
    P.boff[l] = (int)(at + (size_t)P.in[l] * (size_t)policy_padded(P.out[l]));
    at += policy_layer_floats(P.in[l], P.out[l]);
  }
  P.shift_off = (int)at, at += POLICY_NOBS;
  P.scale_off = (int)at, at += POLICY_NOBS;
  P.std_off = (int)at, at += POLICY_MAX_ADIM;
  P.low_off = (int)at, at += POLICY_MAX_ADIM;
  P.high_off = (int)at, at += POLICY_MAX_ADIM;
  return at;
}
// the blob from the caller's arrays (weight[l] row-major [out][in] as torch.nn.Linear.weight; null bias = 0, null
// shift = 0, null scale = 1, null log_std = deterministic (std 0), null low / high = no clamp: -+FLT_MAX);
// `blob` has policy_layout(P) floats
inline void policy_pack(const MmxPolicy& P, const float* const* weight, const float* const* bias, const float* shift,
                        const float* scale, const float* log_std, const float* low, const float* high, float* blob) {
  for (int l = 0; l < P.n_layers; l++) {
    const int in = P.in[l], out = P.out[l], outp = policy_padded(out);
    for (int k = 0; k < in; k++)
      for (int j = 0; j < outp; j++)
        blob[(size_t)P.woff[l] + policy_windex(out, k, j)] = j < out ? weight[l][(size_t)j * (size_t)in + (size_t)k] : 0.f;
    for (int j = 0; j < outp; j++) blob[(size_t)P.boff[l] + (size_t)j] = j < out && bias[l] ? bias[l][j] : 0.f;
  }
  for (int k = 0; k < POLICY_NOBS; k++) {
    blob[P.shift_off + k] = shift ? shift[k] : 0.f;
    blob[P.scale_off + k] = scale ? scale[k] : 1.f;
  }
  for (int a = 0; a < POLICY_MAX_ADIM; a++) {
    blob[P.std_off + a] = log_std && a < P.A ? (float)exp((double)log_std[a]) : 0.f;
    blob[P.low_off + a] = low && a < P.A ? low[a] : -FLT_MAX;
    blob[P.high_off + a] = high && a < P.A ? high[a] : FLT_MAX;
  }
}

// ---- the network's input: two roundings, so a scale of 0 drops a (finite) entry whatever its size
POLICY_HD float policy_normalise(float obs, float shift, float scale) { return (obs - shift) * scale; }

// ---- one neuron: a single fp32 accumulator from the bias, k ascending, fused multiply-adds
POLICY_HD float policy_neuron(const float* w /* the layer's weights */, int out, int in, int j, float bias, const float* x) {
  float acc = bias;
  for (int k = 0; k < in; k++) acc = fmaf(w[policy_windex(out, k, j)], x[k], acc);
  return acc;
}

// ---- the activation.  tanh x = 1 - 2 / (1 + exp2(2 x log2 e)): the exponent's argument is capped at 64, where the
// quotient is already below half an ulp of 1, so no infinity is ever formed (the sources are built
// -ffinite-math-only): exactly +-1 for |x| >= 23, exactly 0 at 0 (exp2(0) = 1, 1 / 2 exact).  The device takes the
// hardware's exp2 and reciprocal (one ulp each); the absolute error stays within 8 * 2^-24.
POLICY_HD float policy_tanh(float x) {
  const float e2 = fminf(x * 2.8853900817779268f, 64.f);
#if defined(__HIP_DEVICE_COMPILE__)
  return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(e2));
#else
  return 1.f - 2.f / (1.f + exp2f(e2));
#endif
}
POLICY_HD float policy_activate(int activation, float x) { return activation == POLICY_RELU ? fmaxf(x, 0.f) : policy_tanh(x); }

// ---- the action component: clamp(std z + mean, low, high), one fused multiply-add
POLICY_HD float policy_action(float mean, float std, float z, float lo, float hi) { return mppi_clamp(fmaf(std, z, mean), lo, hi); }

// ---- scalar reference of the whole forward pass: obs [85] -> mean [A]; buf: 2 * POLICY_MAX_WIDTH + POLICY_NOBS floats
inline void policy_forward_ref(const MmxPolicy& P, const float* blob, const float* obs, float* mean, float* buf) {
  float* x = buf;
  float* pp[2] = {buf + POLICY_NOBS, buf + POLICY_NOBS + POLICY_MAX_WIDTH};
  for (int k = 0; k < POLICY_NOBS; k++) x[k] = policy_normalise(obs[k], blob[P.shift_off + k], blob[P.scale_off + k]);
  const float* src = x;
  for (int l = 0; l < P.n_layers; l++) {
    float* dst = pp[l & 1];
    for (int j = 0; j < P.out[l]; j++) {
      const float v = policy_neuron(blob + P.woff[l], P.out[l], P.in[l], j, blob[P.boff[l] + j], src);
      dst[j] = l + 1 < P.n_layers ? policy_activate(P.activation, v) : v;
    }
    src = dst;
  }
  for (int a = 0; a < P.A; a++) mean[a] = src[a];
}

#if defined(__HIPCC__)
// ---- the wave's forward pass.  All 64 lanes of ONE wave call it with the normalised input in x[0 .. 85) (LDS);
// lane j computes neurons j, j + 64, j + 128, j + 192 of a layer (NQ = outp / 64 independent accumulators: the
// ILP), reads each input from LDS as a broadcast and its weights as coalesced rows; the activations alternate
// between the two LDS buffers b0, b1 [POLICY_MAX_WIDTH].  Returns the buffer that holds the last layer's outputs
// (the mean, [A]); the padding neurons of a layer hold act(0).  A wave's LDS operations complete in order, so the
// layers are joined by a wave-level fence: no workgroup barrier, no atomics.
__device__ __forceinline__ void policy_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// the blob is global memory: said so, the weight reads are global loads off a scalar base, not flat ones
typedef const __attribute__((address_space(1))) float* policy_gptr;
// Wave-uniform values said to be so (scalar registers, scalar branches): a caller that got P by reference
// loads its fields per lane as far as the compiler can tell.  Field by field, never a copy of the struct: its
// arrays, indexed by the layer, would live in scratch memory.
__device__ __forceinline__ int policy_u(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ const float* policy_data(const MmxPolicy& P) {
  const uint64_t d = (uint64_t)(uintptr_t)P.data;
  return (const float*)(uintptr_t)(((uint64_t)(uint32_t)policy_u((int)(uint32_t)(d >> 32)) << 32) | (uint32_t)policy_u((int)(uint32_t)d));
}
template <int NQ>
__device__ __forceinline__ void policy_layer_wave(policy_gptr __restrict__ w, policy_gptr __restrict__ b, int in, bool act,
                                                  int activation, const float* src, float* dst, int lane) {
  constexpr int outp = NQ * POLICY_LANES;
  float acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++) acc[q] = b[q * POLICY_LANES + lane];
  policy_gptr row = w + lane;
#pragma unroll 8
  for (int k = 0; k < in; k++) {
    const float xk = src[k];
#pragma unroll
    for (int q = 0; q < NQ; q++) acc[q] = fmaf(row[q * POLICY_LANES], xk, acc[q]);
    row += outp;
  }
#pragma unroll
  for (int q = 0; q < NQ; q++) dst[q * POLICY_LANES + lane] = act ? policy_activate(activation, acc[q]) : acc[q];
}
__device__ __forceinline__ const float* policy_forward_wave(const MmxPolicy& P, const float* data /* policy_data(P) */,
                                                            const float* x, float* b0, float* b1, int lane) {
  const float* src = x;
  const int n_layers = policy_u(P.n_layers), activation = policy_u(P.activation);
  for (int l = 0; l < n_layers; l++) {
    float* dst = (l & 1) ? b1 : b0;
    const int in = policy_u(P.in[l]), out = policy_u(P.out[l]);
    policy_gptr w = (policy_gptr)(data + policy_u(P.woff[l]));
    policy_gptr b = (policy_gptr)(data + policy_u(P.boff[l]));
    const bool act = l + 1 < n_layers;
    switch (policy_padded(out) / POLICY_LANES) {
      case 1: policy_layer_wave<1>(w, b, in, act, activation, src, dst, lane); break;
      case 2: policy_layer_wave<2>(w, b, in, act, activation, src, dst, lane); break;
      case 3: policy_layer_wave<3>(w, b, in, act, activation, src, dst, lane); break;
      default: policy_layer_wave<4>(w, b, in, act, activation, src, dst, lane); break;
    }
    policy_wave_sync();
    src = dst;
  }
  return src;
}
#endif

#endif
