// The closed forms of the MPPI planner (mmx_mppi_plan, include/mmx_api.h) as host + device inline functions:
// the kernels of mmx_mppi.hip call them, and a stand-alone host program (tests/host/mmx_mppi_selftest.cpp,
// plain g++) runs the very same code.  Philox4x32-10, the draw of one noise element, the beta filter, a
// candidate's return, the finite test, the softmax weight, and a scalar reference of one group's update.
//
// Layouts (i = m * K + k is the planner env of candidate k of controlled env m, N = M * K):
//   nominal [H][M][A]   noise, actions [H][N][A]   reward [H][N]   done [H][N][3]   returns, weights [N]   best [M]
#ifndef MMX_MPPI_H
#define MMX_MPPI_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MPPI_HD __host__ __device__ inline
#else
#define MPPI_HD inline
#endif

#define MPPI_MAX_HORIZON 64  // MMX_MPPI_MAX_HORIZON
#define MPPI_MAX_ADIM 10     // MMX_MPPI_MAX_ADIM

// What a launch needs of the planner's configuration (by value: kernel arguments).  The per-component
// sigma / low / high are a device array `box` [3][MPPI_MAX_ADIM] instead (indexed by a thread's component).
struct MppiParams {
  int H, M, K, A;
  float inv_lambda;  // 1 / temperature; 0: temperature 0 (one-hot on the best candidate)
  float gamma;
  float beta, beta_c;  // noise_beta and sqrt(1 - beta^2)
  uint32_t seed_lo, seed_hi, call_lo, call_hi;
};
struct MppiBufs {
  float* nominal;
  float* noise;
  float* actions;
  float* reward;
  int* done;
  float* returns;
  float* weights;
  int* best;
};

// ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
MPPI_HD void mppi_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// ---- the draw.  Element (t, i, a) of call `call` under `seed`: key = (seed low, seed high), counter =
// (call low, call high, i, 4 t + a / 4); of the block's outputs x0..x3 component a uses the pair (x0, x1)
// when a % 4 < 2 and (x2, x3) otherwise: u1 = ((x >> 8) + 1) 2^-24 in (0, 1], u2 = (x' >> 8) 2^-24 in [0, 1).
MPPI_HD void mppi_draw_uniforms(uint32_t seed_lo, uint32_t seed_hi, uint32_t call_lo, uint32_t call_hi, uint32_t t,
                                uint32_t i, uint32_t a, float* u1, float* u2) {
  const uint32_t ctr[4] = {call_lo, call_hi, i, 4u * t + a / 4u}, key[2] = {seed_lo, seed_hi};
  uint32_t x[4];
  mppi_philox4x32_10(ctr, key, x);
  const bool second = (a & 2u) != 0u;
  const uint32_t xa = second ? x[2] : x[0], xb = second ? x[3] : x[1];
  *u1 = (float)((xa >> 8) + 1u) * 5.9604644775390625e-08f;
  *u2 = (float)(xb >> 8) * 5.9604644775390625e-08f;
}
// Box-Muller: sqrt(-2 ln u1) cos 2 pi u2 (even a) or sin (odd a).  The device takes the hardware's log2, and
// its sine / cosine of an angle given in revolutions; the host evaluates in double with libm.
MPPI_HD float mppi_box_muller(float u1, float u2, bool odd) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float r = __builtin_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));  // -2 ln 2 log2 u1
  return r * (odd ? __builtin_amdgcn_sinf(u2) : __builtin_amdgcn_cosf(u2));
#else
  const double r = sqrt(-2.0 * log((double)u1)), ang = 6.283185307179586476925 * (double)u2;
  return (float)(r * (odd ? sin(ang) : cos(ang)));
#endif
}
MPPI_HD float mppi_draw(uint32_t seed_lo, uint32_t seed_hi, uint32_t call_lo, uint32_t call_hi, uint32_t t, uint32_t i,
                        uint32_t a) {
  float u1, u2;
  mppi_draw_uniforms(seed_lo, seed_hi, call_lo, call_hi, t, i, a, &u1, &u2);
  return mppi_box_muller(u1, u2, (a & 1u) != 0u);
}

// ---- the beta filter: eps_0 = xi_0, eps_t = beta eps_{t-1} + sqrt(1 - beta^2) xi_t (beta_c = the root)
MPPI_HD float mppi_filter(float beta, float beta_c, float eps_prev, float xi) { return fmaf(beta, eps_prev, beta_c * xi); }

// ---- a candidate's action component
MPPI_HD float mppi_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }
MPPI_HD float mppi_action(float nominal, float sigma, float eps, float lo, float hi) {
  return mppi_clamp(fmaf(sigma, eps, nominal), lo, hi);
}

// ---- the finite test, on the bits.  mmx_mppi.hip is built with NaN / Inf semantics (_build.SOURCE_FLAGS): under
// the other sources' -ffinite-math-only the compiler folds this to true for a value it saw computed
MPPI_HD bool mppi_finite(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return (u & 0x7F800000u) != 0x7F800000u;
}

// ---- R_i = sum_t gamma^t reward[t][i] alive_t, alive_0 = 1, alive_{t+1} = alive_t and not (terminated_t or
// truncated_t): the ending step's reward counts, nothing after it is even read into the sum
MPPI_HD float mppi_return(const float* reward, const int* done, size_t N, size_t i, int H, float gamma) {
  float R = 0.f, g = 1.f;
  for (int t = 0; t < H; t++) {
    const size_t e = (size_t)t * N + i;
    R = fmaf(g, reward[e], R);
    if (done[3 * e] | done[3 * e + 1]) break;
    g *= gamma;
  }
  return R;
}

// ---- the unnormalised weight of a finite return under temperature > 0: exp((R - max R) / lambda) <= 1
MPPI_HD float mppi_weight(float R, float Rmax, float inv_lambda) {
  const float x = (R - Rmax) * inv_lambda;
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_exp2f(x * 1.4426950408889634f);  // x <= 0: a result below the normal range is 0
#else
  return expf(x);
#endif
}
// is candidate (Ra, ka) a better maximum than (Rb, kb)?  k < 0: no candidate; ties go to the lower k
MPPI_HD bool mppi_better(float Ra, int ka, float Rb, int kb) {
  return ka >= 0 && (kb < 0 || Ra > Rb || (Ra == Rb && ka < kb));
}

// ---- scalar reference of one group's update (controlled env m), in ascending k: what
// mmx_mppi_update_kernel computes with its sums in another (fixed) order.  box = [3][MPPI_MAX_ADIM]
// sigma, low, high.  A wholly excluded group: weights 0, best -1, the nominal kept (not shifted) and
// action_out = its first step.
inline void mppi_group_update_ref(const MppiParams& P, const MppiBufs& B, const float* box, int m, float* action_out) {
  const size_t K = (size_t)P.K, N = (size_t)P.M * K, i0 = (size_t)m * K, A = (size_t)P.A, M = (size_t)P.M;
  float Rmax = 0.f;
  int best = -1;
  for (size_t k = 0; k < K; k++) {
    const float R = mppi_return(B.reward, B.done, N, i0 + k, P.H, P.gamma);
    B.returns[i0 + k] = R;
    if (mppi_finite(R) && mppi_better(R, (int)k, Rmax, best)) Rmax = R, best = (int)k;
  }
  B.best[m] = best;
  if (best < 0) {
    for (size_t k = 0; k < K; k++) B.weights[i0 + k] = 0.f;
    for (size_t a = 0; a < A; a++) action_out[(size_t)m * A + a] = B.nominal[(size_t)m * A + a];
    return;
  }
  float sum = 0.f;
  for (size_t k = 0; k < K; k++) {
    const float R = B.returns[i0 + k];
    float e = 0.f;
    if (mppi_finite(R)) e = P.inv_lambda > 0.f ? mppi_weight(R, Rmax, P.inv_lambda) : ((int)k == best ? 1.f : 0.f);
    B.weights[i0 + k] = e;
    sum += e;
  }
  const float inv = 1.f / sum;
  for (size_t k = 0; k < K; k++) B.weights[i0 + k] *= inv;
  float fresh[MPPI_MAX_HORIZON * MPPI_MAX_ADIM];
  for (size_t t = 0; t < (size_t)P.H; t++)
    for (size_t a = 0; a < A; a++) {
      float acc = 0.f;
      for (size_t k = 0; k < K; k++) acc = fmaf(B.weights[i0 + k], B.actions[(t * N + i0 + k) * A + a], acc);
      fresh[t * A + a] = mppi_clamp(acc, box[MPPI_MAX_ADIM + a], box[2 * MPPI_MAX_ADIM + a]);
    }
  for (size_t t = 0; t < (size_t)P.H; t++) {
    const size_t from = t + 1 < (size_t)P.H ? t + 1 : t;
    for (size_t a = 0; a < A; a++) B.nominal[(t * M + (size_t)m) * A + a] = fresh[from * A + a];
  }
  for (size_t a = 0; a < A; a++) action_out[(size_t)m * A + a] = fresh[a];
}

#endif
