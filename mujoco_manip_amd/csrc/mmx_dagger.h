// The closed forms of the DAgger rollout's gate (mmx_rollout_dagger, include/mmx_api.h) as host + device inline
// functions: mmx_env_dagger_kernel (mmx_step_kernels.inc) calls them, and a stand-alone host program
// (tests/host/mmx_dagger_selftest.cpp, plain g++) runs the very same code.  The gate's uniform draw, the Bernoulli
// gate, the takeover distance and predicate, the gate word and the executed action.
//
// Per rollout step t and env i the learner's action a_policy [4] (mmx_policy.h: mean, noise, clamp) and the FSM
// expert's a_expert [4] are both known; gate = bern | take << 1 decides which one the env is stepped with:
//   bern   u < beta, u the second uniform of mppi_draw_uniforms(policy seed, call, t, i, a = 12): counter word
//          4 t + 3, the block no noise component uses (a < MPPI_MAX_ADIM = 10 stays in words 4 t .. 4 t + 2), so the
//          gate is independent of the noise; u = (x1 >> 8) 2^-24 lies in [0, 1): beta = 0 never fires, 1 always
//   take   takeover_dist > 0 and |a_policy - a_expert|^2 over xyz > takeover_dist^2: the expert intervenes when
//          the learner strays; takeover_dist = 0 switches it off
// The executed action is the expert's (all four components) when gate != 0, else the learner's.
#ifndef MMX_DAGGER_H
#define MMX_DAGGER_H
#include "mmx_mppi.h"

#define DAGGER_HD MPPI_HD
#define DAGGER_GATE_COMPONENT 12u  // the draw's component index: block 3 of the step's four Philox counter words
#define DAGGER_BERNOULLI 1         // gate bit 0
#define DAGGER_TAKEOVER 2          // gate bit 1
static_assert(DAGGER_GATE_COMPONENT / 4u == 3u && MPPI_MAX_ADIM <= 12, "the gate's counter word is one a noise component uses");

// What a launch needs of the gate and of the DAgger record (by value: kernel arguments).  Device arrays
// [T][N][4] but gate [T][N] and obs_in [T][N][85]; policy_action is the hand-off row policy_act writes and is never
// null here (mmx_rollout_dagger passes `actions` for it when the caller records no policy_action: lane 0 reads the
// learner's row before it writes the executed one); expert_action, gate and obs_in may be null.
struct MMXDagger {
  float* actions;
  float* expert_action;
  float* policy_action;
  int* gate;
  float* obs_in;
  float beta, takeover_dist;
};

// ---- the gate's uniform of (seed, call, t, i): in [0, 1), 24 bits
DAGGER_HD float dagger_uniform(uint32_t seed_lo, uint32_t seed_hi, uint32_t call_lo, uint32_t call_hi, uint32_t t, uint32_t i) {
  float u1, u2;
  mppi_draw_uniforms(seed_lo, seed_hi, call_lo, call_hi, t, i, DAGGER_GATE_COMPONENT, &u1, &u2);
  return u2;
}
DAGGER_HD int dagger_bernoulli(float u, float beta) { return u < beta ? 1 : 0; }

// ---- the takeover: squared xyz distance in fp32, x first, then fused multiply-adds
DAGGER_HD float dagger_dist2(const float* a_policy, const float* a_expert) {
  const float dx = a_policy[0] - a_expert[0], dy = a_policy[1] - a_expert[1], dz = a_policy[2] - a_expert[2];
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}
DAGGER_HD int dagger_takeover(float d2, float takeover_dist) {
  return takeover_dist != 0.f && d2 > takeover_dist * takeover_dist ? 1 : 0;
}

// ---- the gate word and the executed action
DAGGER_HD int dagger_gate(float u, float beta, const float* a_policy, const float* a_expert, float takeover_dist) {
  return dagger_bernoulli(u, beta) | dagger_takeover(dagger_dist2(a_policy, a_expert), takeover_dist) << 1;
}
DAGGER_HD void dagger_select(int gate, const float* a_policy, const float* a_expert, float* out4) {
  for (int k = 0; k < 4; k++) out4[k] = gate ? a_expert[k] : a_policy[k];
}

#endif
