// The closed forms of the policy-gradient fit (mmx_gae, mmx_policy_fit_pg, include/mmx_api.h) as host + device inline
// functions: the kernels of mmx_policy_fit.hip call them, and a stand-alone host program
// (tests/host/mmx_pg_selftest.cpp, plain g++) runs the very same code.  Generalised advantage estimation over a
// rollout record, the normalisation's two sums, PPO's clipped surrogate as an output delta of the training step of
// mmx_policy_fit.h, and a scalar reference of one whole step.  Every line below is one rounding; the functions are
// compiled with floating-point contraction off, and mmx_policy_fit.hip with IEEE division (SOURCE_FLAGS, _build.py).
//
// GAE(lambda), one env column i, t from T - 1 down to 0 (Schulman et al. 2016):
//   term  = done[t][i][0] != 0
//   end   = term || done[t][i][1] != 0          every autoreset carries a done flag (step_finish)
//   nv    = end ? 0 : (t == T - 1 ? value_last[i] : value[t + 1][i])
//   delta = fmaf(gamma, nv, reward[t][i]) - value[t][i]
//   adv   = end ? delta : fmaf(gl, adv_next, delta)       gl = gamma * lambda, one fp32 product made on the host
//   ret   = adv + value[t][i]
// value[t][i] = V of the observation the env held before step t, value_last[i] = V of the observation after the last
// step.  A truncated step takes next value 0, like a terminated one: the record keeps the new episode's first
// observation, not the ended episode's last one (mmx_rollout_actions, include/mmx_api.h), so V of the state the
// truncation cut off cannot be evaluated from a record; bootstrapping from value[t + 1] would take the value of a
// state of another episode.  What lies behind an ended step never reaches it: `end` drops both nv and adv_next.
//
// Normalisation over all n = T N advantages: mean = S1 / n, var = S2 / n with S2 = sum (x - mean)^2, adv = (adv - mean)
// / (sqrtf(var) + 1e-8f).  The shape of both sums is fixed by n alone (pg_sum below): PG_SUM_LANES strided chains,
// chain i = elements i, i + PG_SUM_LANES, .. ascending, plain adds from 0; then a binary tree over the chains,
// strides PG_SUM_LANES / 2 .. 1, chain[i] += chain[i + stride].  No floating-point atomics.
//
// PPO's clipped surrogate (Schulman et al. 2017), sample s with pair p, sigma_a = the blob's std entry (> 0):
//   u_a   = fmaf(sigma_a, noise[p][a], mean_old[p][a])      the pre-clamp sample: policy_action's own expression
//   z'_a  = (u_a - mean'_a) / sigma_a                       mean' = the network's output now
//   lr_s  = sum_{a < A, ascending} fmaf(0.5, fmaf(-z'_a, z'_a, z_a z_a), lr)     z_a = noise[p][a]; log of the ratio
//   r_s   = expf(lr_s)
//   live  = !((Adv_p > 0 && r_s > hi) || (Adv_p < 0 && r_s < lo))        lo = 1 - clip, hi = 1 + clip, fp32, host
//   loss_s = -fminf(r_s Adv_p, clampf(r_s, lo, hi) Adv_p)
//   d[s][a] = live ? -(((invB Adv_p) r_s) (z'_a / sigma_a)) : 0          invB = 1 / B, from the host
// The log-probability is that of the pre-clamp sample: the clamp is part of the environment.  With sigma fixed the
// ratio needs nothing but mean_old and noise, which mmx_policy_record holds; log_std is not trained.
// Statistics of a step: loss = invB sum_s loss_s, approximate KL = invB sum_s ((r_s - 1) - lr_s), clipped fraction =
// invB sum_s !live; each sum runs over the samples of a tile of FIT_TS in order, then over the tiles in order.
#ifndef MMX_PG_H
#define MMX_PG_H
#include "mmx_policy_fit.h"

#define PG_SUM_LANES 1024   // the chains of pg_sum = the threads of the one workgroup that sums
#define PG_NORM_EPS 1e-8f

// What the forward launch of a PG step needs besides MmxFit (by value: a kernel argument of its own, so MmxFit and
// the three kernels that take it stay as they are).  F.target is unused.  stat_base: a float offset into F.ws
struct MmxPg {
  const float* mean_old;  // [n][A]
  const float* noise;     // [n][A]
  const float* adv;       // [n]
  size_t stat_base;       // [tiles][3] partials: loss, kl, clipped
  float invB, lo, hi;     // 1 / B, 1 - clip, 1 + clip
};
inline float pg_inv_batch(int B) { return 1.f / (float)B; }

// ---- GAE: one step of the backward recursion of a column; returns adv[t], *ret = adv + value
POLICY_HD float pg_gae_step(float gamma, float gl, int term, int trunc, float reward, float value, float next_value,
                            float adv_next, float* ret) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool end = term != 0 || trunc != 0;
  const float nv = end ? 0.f : next_value;
  const float delta = fmaf(gamma, nv, reward) - value;
  const float adv = end ? delta : fmaf(gl, adv_next, delta);
  *ret = adv + value;
  return adv;
}
// the whole record on the host: the kernel's loop, one column after the other
inline void pg_gae_ref(float gamma, float lambda, int T, int N, const float* reward, const int32_t* done, const float* value,
                       const float* value_last, float* adv_out, float* ret_out /* or null */) {
  const float gl = gamma * lambda;
  for (int i = 0; i < N; i++) {
    float adv = 0.f;
    for (int t = T - 1; t >= 0; t--) {
      const size_t e = (size_t)t * (size_t)N + (size_t)i;
      const float nv = t == T - 1 ? value_last[i] : value[e + (size_t)N];
      float ret;
      adv = pg_gae_step(gamma, gl, done[3 * e], done[3 * e + 1], reward[e], value[e], nv, adv, &ret);
      adv_out[e] = adv;
      if (ret_out) ret_out[e] = ret;
    }
  }
}

// ---- the normalisation.  One term of a sum: x itself, or (x - mean)^2 (two roundings)
POLICY_HD float pg_sum_term(float x, float mean, int square) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!square) return x;
  const float c = x - mean;
  return c * c;
}
// the sum in the shape stated at the head of this file (host: the kernel's order, lane by lane)
inline float pg_sum(const float* x, int64_t n, float mean, int square) {
  std::vector<float> chain(PG_SUM_LANES, 0.f);
  for (int64_t e = 0; e < n; e++) chain[(size_t)(e % PG_SUM_LANES)] += pg_sum_term(x[e], mean, square);
  for (int stride = PG_SUM_LANES / 2; stride >= 1; stride >>= 1)
    for (int i = 0; i < stride; i++) chain[(size_t)i] += chain[(size_t)(i + stride)];
  return chain[0];
}
POLICY_HD float pg_norm_denominator(float s2, float n) { return sqrtf(s2 / n) + PG_NORM_EPS; }
POLICY_HD float pg_normalise(float x, float mean, float den) { return (x - mean) / den; }
inline void pg_normalise_ref(float* adv, int64_t n) {
  const float mean = pg_sum(adv, n, 0.f, 0) / (float)n;
  const float den = pg_norm_denominator(pg_sum(adv, n, mean, 1), (float)n);
  for (int64_t e = 0; e < n; e++) adv[e] = pg_normalise(adv[e], mean, den);
}

// ---- PPO: one component's share of a sample
POLICY_HD float pg_znew(float std, float z, float mean_old, float mean) {
  const float u = fmaf(std, z, mean_old);
  const float c = u - mean;
  return c / std;
}
// lr + 0.5 (z^2 - z'^2), the terms in ascending a
POLICY_HD float pg_log_ratio_add(float lr, float z, float zn) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float zz = z * z;
  const float dd = fmaf(-zn, zn, zz);
  return fmaf(0.5f, dd, lr);
}
// what a sample's ratio decides, once per sample: g = the factor of every component's delta (0 when clipped), and the
// sample's three statistics
struct PgSample { float g, loss, kl, clipped; };
POLICY_HD PgSample pg_sample(float lr, float adv, float invB, float lo, float hi) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float r = expf(lr);
  const bool live = !((adv > 0.f && r > hi) || (adv < 0.f && r < lo));
  const float ra = r * adv;
  const float ca = fminf(fmaxf(r, lo), hi) * adv;
  const float w = invB * adv;
  const float rm1 = r - 1.f;
  PgSample o;
  o.g = live ? w * r : 0.f;
  o.loss = -fminf(ra, ca);
  o.kl = rm1 - lr;
  o.clipped = live ? 0.f : 1.f;
  return o;
}
POLICY_HD float pg_out_delta(float g, float zn, float std) {
  const float q = zn / std;
  return -(g * q);
}

// ---- scalar reference of one whole PG step: policy_step_ref (mmx_policy_fit.h: the batch, the forward pass, the
// hidden deltas, the gradient sums and the update) with the output delta above.  stats [3] = loss, approximate KL,
// clipped fraction of the batch before the update, summed tile by tile as the kernel does.
inline void policy_pg_step_ref(const MmxPolicy& P, float* blob, const float* obs, const float* mean_old, const float* noise,
                               const float* adv, int64_t n, int B, int shuffle, uint64_t seed, uint64_t k, float clip,
                               const MmxFitOpt& opt, float* m, float* v, float* stats) {
  const int A = P.A;
  const float invB = pg_inv_batch(B), lo = 1.f - clip, hi = 1.f + clip;
  float total[3] = {0.f, 0.f, 0.f}, tile[3] = {0.f, 0.f, 0.f};
  float zn[POLICY_MAX_ADIM];
  policy_step_ref(P, blob, obs, n, B, shuffle, seed, k, opt, m, v, [&](int s, int64_t p, const float* mean, float* d) {
    float lr = 0.f;
    for (int a = 0; a < A; a++) {
      const size_t e = (size_t)p * (size_t)A + (size_t)a;
      zn[a] = pg_znew(blob[P.std_off + a], noise[e], mean_old[e], mean[a]);
      lr = pg_log_ratio_add(lr, noise[e], zn[a]);
    }
    const PgSample q = pg_sample(lr, adv[p], invB, lo, hi);
    for (int a = 0; a < A; a++) d[a] = pg_out_delta(q.g, zn[a], blob[P.std_off + a]);
    tile[0] += q.loss, tile[1] += q.kl, tile[2] += q.clipped;
    if ((s + 1) % FIT_TS == 0 || s + 1 == B)
      for (int c = 0; c < 3; c++) total[c] += tile[c], tile[c] = 0.f;
  });
  for (int c = 0; c < 3; c++) stats[c] = total[c] * invB;
}

#endif
