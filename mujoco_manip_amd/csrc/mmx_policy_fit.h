// The closed forms of the MLP policy's training step (mmx_policy_fit, include/mmx_api.h) as host + device inline
// functions: the kernels of mmx_policy_fit.hip call them, and a stand-alone host program
// (tests/host/mmx_policy_fit_selftest.cpp, plain g++) runs the very same code.  The batch's pair indices, the output
// and hidden deltas, the two optimisers, and a scalar reference of one whole step on the packed blob of mmx_policy.h.
//
// The loss of a batch of B pairs (x_s, y_s):  L = 1 / (B A) sum_{s, a} (mean(x_s)[a] - y_s[a])^2, mean = the network
// of policy_forward_ref (before noise and clamp).  Its gradient:
//   output delta     d_{L-1}[s][a] = 2 / (B A) (mean[s][a] - y[s][a])
//   hidden delta     d_l[s][k] = (sum_j W_{l+1}[j][k] d_{l+1}[s][j]) act'(a_l[s][k]), j ascending from 0, fused
//                    multiply-adds; act' from the saved activation a: tanh 1 - a^2 = fma(-a, a, 1), ReLU a > 0
//   dW_l[j][k] = sum_s x_l[s][k] d_l[s][j],  db_l[j] = sum_s d_l[s][j]  (x_0 = the normalised observation,
//                    x_l = a_{l-1}); the bias is the weight of a constant input 1, which is how the blob stores it
//                    (row in_l of the [in_l + 1][outp_l] matrix that starts at woff_l), and how the kernels sum it
// obs_shift, obs_scale, std, low and high are not trained.
//
// The batch.  Sample s of optimisation step k (k = t - 1, the policy's running step counter) is pair
//   shuffle 0:  (k B + s) mod n                                   (64-bit arithmetic)
//   shuffle 1:  (uint64(x) n) >> 32, x = word s % 4 of Philox4x32-10 with key = (seed low, seed high) and counter =
//               (k low, k high, s / 4, FIT_DOMAIN): a function of (seed, k, s) alone.  The whole 32-bit word, not the
//               24-bit uniform of the noise draws: n goes up to 2^31 - 1.  FIT_DOMAIN keeps these counters apart from
//               every noise draw of a policy with the same seed (whose 4th word is 4 t + a / 4 < 2^31 there).
//
// The optimisers, one scalar weight w with gradient g; every line is one rounding, nothing else is fused (the
// functions are compiled with floating-point contraction off):
//   MMX_FIT_SGD    w = fma(-lr, g, w)
//   MMX_FIT_ADAM   m = fma(beta1, m, omb1 g)             omb1 = 1 - beta1 (fp32, host)
//                  v = fma(beta2, v, (omb2 g) g)         omb2 = 1 - beta2 (fp32, host)
//                  mhat = m c1,  vhat = v c2             c1 = 1 / (1 - beta1^t), c2 = 1 / (1 - beta2^t): evaluated once
//                                                        per step on the host in fp64, rounded to fp32
//                  w = w - (lr mhat) / (sqrt(vhat) + eps)   correctly rounded sqrt and division
#ifndef MMX_POLICY_FIT_H
#define MMX_POLICY_FIT_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "mmx_policy.h"

#define FIT_SGD 0              // MMX_FIT_SGD
#define FIT_ADAM 1             // MMX_FIT_ADAM
#define FIT_MAX_BATCH 65536    // MMX_FIT_MAX_BATCH
#define FIT_DOMAIN 0xF17BA7C4u  // the 4th counter word of the batch draws

#define FIT_TS 16    // samples per workgroup of the forward / delta kernel
#define FIT_KC 512   // samples per K chunk of the weight-gradient GEMM (one partial each)

// What the launches of one optimisation step need besides the policy (by value: kernel arguments).  ws = the
// workspace (layout: mmx_policy_fit.hip), the three bases are float offsets into it
struct MmxFit {
  const float* obs;     // [n][85]
  const float* target;  // [n][A]
  int64_t n;
  float* ws;
  size_t d_base, loss_base, part_base;
  uint64_t k;  // the running step counter, t - 1
  uint32_t seed_lo, seed_hi;
  int B, shuffle;
  float dscale, inv_count;  // 2 / (B A), 1 / (B A)
};

// One optimisation step's scalars (by value: kernel arguments), all prepared on the host
struct MmxFitOpt {
  int optimizer;
  float lr, beta1, omb1, beta2, omb2, c1, c2, eps;
};
inline MmxFitOpt policy_fit_opt(int optimizer, float lr, float beta1, float beta2, float eps, uint64_t t /* >= 1 */) {
  MmxFitOpt o{optimizer, lr, beta1, 1.f - beta1, beta2, 1.f - beta2, 1.f, 1.f, eps};
  o.c1 = (float)(1.0 / (1.0 - pow((double)beta1, (double)t)));
  o.c2 = (float)(1.0 / (1.0 - pow((double)beta2, (double)t)));
  return o;
}
// 1 / (B A) and the output delta's factor 2 / (B A), fp32 (host: an IEEE division; the kernels get them as arguments)
inline float policy_fit_inv_count(int B, int A) { return 1.f / (float)((int64_t)B * A); }

// ---- the batch's pair index
POLICY_HD int64_t policy_fit_index(int shuffle, uint32_t seed_lo, uint32_t seed_hi, uint64_t k, uint32_t s, uint32_t B,
                                   int64_t n) {
  if (!shuffle) return (int64_t)((k * (uint64_t)B + (uint64_t)s) % (uint64_t)n);
  const uint32_t ctr[4] = {(uint32_t)k, (uint32_t)(k >> 32), s / 4u, FIT_DOMAIN}, key[2] = {seed_lo, seed_hi};
  uint32_t x[4];
  mppi_philox4x32_10(ctr, key, x);
  const uint32_t w = (s & 3u) == 0u ? x[0] : (s & 3u) == 1u ? x[1] : (s & 3u) == 2u ? x[2] : x[3];
  return (int64_t)(((uint64_t)w * (uint64_t)n) >> 32);
}

// ---- the deltas
POLICY_HD float policy_fit_out_delta(float mean, float y, float dscale /* 2 / (B A) */) { return dscale * (mean - y); }
POLICY_HD float policy_fit_act_grad(int activation, float a /* the saved activation */) {
  return activation == POLICY_RELU ? (a > 0.f ? 1.f : 0.f) : fmaf(-a, a, 1.f);
}
// one hidden delta: `back` = the sum over the next layer, a = this unit's saved activation
POLICY_HD float policy_fit_hidden_delta(int activation, float back, float a) { return back * policy_fit_act_grad(activation, a); }

// ---- the optimisers (operation order: the head of this file)
POLICY_HD float policy_fit_sgd(float w, float g, float lr) { return fmaf(-lr, g, w); }
POLICY_HD float policy_fit_adam(float w, float g, float* m, float* v, const MmxFitOpt& o) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float t1 = o.omb1 * g;
  const float mn = fmaf(o.beta1, *m, t1);
  const float t2 = o.omb2 * g;
  const float t3 = t2 * g;
  const float vn = fmaf(o.beta2, *v, t3);
  *m = mn;
  *v = vn;
  const float mhat = mn * o.c1;
  const float vhat = vn * o.c2;
  const float den = sqrtf(vhat) + o.eps;
  const float num = o.lr * mhat;
  const float step = num / den;
  return w - step;
}
POLICY_HD float policy_fit_update(float w, float g, float* m, float* v, const MmxFitOpt& o) {
  return o.optimizer == FIT_ADAM ? policy_fit_adam(w, g, m, v, o) : policy_fit_sgd(w, g, o.lr);
}

// floats of all layers of the blob (weights and biases, padding included): the trained region [0, shift_off),
// and the size of the optimiser's m and v arrays, which are indexed like the blob
inline size_t policy_fit_param_floats(const MmxPolicy& P) { return (size_t)P.shift_off; }

// ---- scalar reference of one whole step in fp32 on the packed blob: the batch gathered by policy_fit_index, the
// forward pass of policy_forward_ref with every layer's activations kept, the deltas, the gradients summed over the
// batch in index order (one fused multiply-add chain from 0 per weight), and the update of every real weight and
// bias.  The padding columns are neither read into a sum nor written: they stay exactly 0.  m, v:
// policy_fit_param_floats(P) floats, indexed like the blob (untouched by SGD).
// The objective is the caller's: out_delta(s, p, mean, d) gets sample s (pair p) with the network's output mean [A],
// writes the output delta d [A] and keeps whatever it sums (the loss, the statistics), samples in order.
template <class OutDelta>
inline void policy_step_ref(const MmxPolicy& P, float* blob, const float* obs, int64_t n, int B, int shuffle, uint64_t seed,
                            uint64_t k, const MmxFitOpt& opt, float* m, float* v, OutDelta&& out_delta) {
  const int L = P.n_layers, A = P.A;
  // x[l]: the input of layer l, [B][in_l]; x[L]: the mean; d[l]: [B][out_l]
  std::vector<std::vector<float>> x((size_t)L + 1), d((size_t)L);
  x[0].resize((size_t)B * POLICY_NOBS);
  for (int l = 0; l < L; l++) x[(size_t)l + 1].resize((size_t)B * (size_t)P.out[l]), d[(size_t)l].resize((size_t)B * (size_t)P.out[l]);
  for (int s = 0; s < B; s++) {
    const int64_t p = policy_fit_index(shuffle, (uint32_t)seed, (uint32_t)(seed >> 32), k, (uint32_t)s, (uint32_t)B, n);
    for (int c = 0; c < POLICY_NOBS; c++)
      x[0][(size_t)s * POLICY_NOBS + (size_t)c] = policy_normalise(obs[(size_t)p * POLICY_NOBS + (size_t)c], blob[P.shift_off + c], blob[P.scale_off + c]);
    for (int l = 0; l < L; l++) {
      const float* src = &x[(size_t)l][(size_t)s * (size_t)P.in[l]];
      float* dst = &x[(size_t)l + 1][(size_t)s * (size_t)P.out[l]];
      for (int j = 0; j < P.out[l]; j++) {
        const float val = policy_neuron(blob + P.woff[l], P.out[l], P.in[l], j, blob[P.boff[l] + j], src);
        dst[j] = l + 1 < L ? policy_activate(P.activation, val) : val;
      }
    }
    out_delta(s, p, &x[(size_t)L][(size_t)s * (size_t)A], &d[(size_t)L - 1][(size_t)s * (size_t)A]);
    for (int l = L - 2; l >= 0; l--) {
      const int out = P.out[l], nout = P.out[l + 1];
      const float* w = blob + P.woff[l + 1];
      for (int c = 0; c < out; c++) {
        float back = 0.f;
        for (int j = 0; j < nout; j++) back = fmaf(w[policy_windex(nout, c, j)], d[(size_t)l + 1][(size_t)s * (size_t)nout + (size_t)j], back);
        d[(size_t)l][(size_t)s * (size_t)out + (size_t)c] = policy_fit_hidden_delta(P.activation, back, x[(size_t)l + 1][(size_t)s * (size_t)out + (size_t)c]);
      }
    }
  }
  for (int l = 0; l < L; l++) {
    const int in = P.in[l], out = P.out[l];
    for (int c = 0; c <= in; c++)  // c == in: the bias
      for (int j = 0; j < out; j++) {
        float g = 0.f;
        for (int s = 0; s < B; s++)
          g = fmaf(c < in ? x[(size_t)l][(size_t)s * (size_t)in + (size_t)c] : 1.f, d[(size_t)l][(size_t)s * (size_t)out + (size_t)j], g);
        const size_t at = (size_t)P.woff[l] + policy_windex(out, c, j);
        blob[at] = policy_fit_update(blob[at], g, m + at, v + at, opt);
      }
  }
}
// The mean-squared error's step.  Returns the batch loss before the update: the squared errors summed in (s, a)
// order, one fused chain, times 1 / (B A).
inline float policy_fit_step_ref(const MmxPolicy& P, float* blob, const float* obs, const float* target, int64_t n, int B,
                                 int shuffle, uint64_t seed, uint64_t k, const MmxFitOpt& opt, float* m, float* v) {
  const int A = P.A;
  const float inv = policy_fit_inv_count(B, A), dscale = 2.f * inv;
  float sq = 0.f;
  policy_step_ref(P, blob, obs, n, B, shuffle, seed, k, opt, m, v, [&](int, int64_t p, const float* mean, float* d) {
    for (int a = 0; a < A; a++) {
      const float y = target[(size_t)p * (size_t)A + (size_t)a], e = mean[a] - y;
      sq = fmaf(e, e, sq);
      d[a] = policy_fit_out_delta(mean[a], y, dscale);
    }
  });
  return sq * inv;
}

#endif
