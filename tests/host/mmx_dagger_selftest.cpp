// Stand-alone host program over csrc/mmx_dagger.h, the closed forms of the DAgger rollout's gate that
// mmx_env_dagger_kernel runs (built by tests/test_dagger_host.py with g++ and AddressSanitizer +
// UndefinedBehaviorSanitizer, run as a child process).  It prints JSON lines that the test compares with its own
// restatements:
//   mmx_dagger_selftest draw (seed call t i)...         the gate's uniform of each group, as a bit pattern, and the
//                                                       two uniforms of every noise component a < 10 of the same
//                                                       (t, i) (mppi_draw_uniforms), as bit patterns
//   mmx_dagger_selftest gate (seed call t i beta tau p0 p1 p2 p3 e0 e1 e2 e3)...
//                                                       u, the Bernoulli bit, d2, the takeover bit, the gate word
//                                                       and the executed action of each group (floats as bit patterns)
// Exit status 2: bad usage.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../mujoco_manip_amd/csrc/mmx_dagger.h"

static uint32_t bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}

struct Key {
  uint32_t seed_lo, seed_hi, call_lo, call_hi, t, i;
};
static Key key(char** a) {
  const uint64_t seed = strtoull(a[0], nullptr, 0), call = strtoull(a[1], nullptr, 0);
  return Key{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)call, (uint32_t)(call >> 32), (uint32_t)strtoul(a[2], nullptr, 0),
             (uint32_t)strtoul(a[3], nullptr, 0)};
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "draw") && (argc - 2) % 4 == 0) {
    for (int k = 2; k + 3 < argc; k += 4) {
      const Key K = key(argv + k);
      const float u = dagger_uniform(K.seed_lo, K.seed_hi, K.call_lo, K.call_hi, K.t, K.i);
      printf("{\"kind\": \"draw\", \"u\": %" PRIu32 ", \"noise\": [", bits(u));
      for (uint32_t a = 0; a < MPPI_MAX_ADIM; a++) {
        float u1, u2;
        mppi_draw_uniforms(K.seed_lo, K.seed_hi, K.call_lo, K.call_hi, K.t, K.i, a, &u1, &u2);
        printf("%s%" PRIu32 ", %" PRIu32, a ? ", " : "", bits(u1), bits(u2));
      }
      printf("]}\n");
    }
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "gate") && (argc - 2) % 14 == 0) {
    for (int k = 2; k + 13 < argc; k += 14) {
      const Key K = key(argv + k);
      float v[10];
      for (int j = 0; j < 10; j++) v[j] = strtof(argv[k + 4 + j], nullptr);
      const float beta = v[0], tau = v[1], *pol = v + 2, *lab = v + 6;
      const float u = dagger_uniform(K.seed_lo, K.seed_hi, K.call_lo, K.call_hi, K.t, K.i);
      const float d2 = dagger_dist2(pol, lab);
      const int gate = dagger_gate(u, beta, pol, lab, tau);
      float act[4];
      dagger_select(gate, pol, lab, act);
      printf("{\"kind\": \"gate\", \"u\": %" PRIu32 ", \"bern\": %d, \"d2\": %" PRIu32 ", \"take\": %d, \"gate\": %d, \"action\": [%" PRIu32
             ", %" PRIu32 ", %" PRIu32 ", %" PRIu32 "]}\n",
             bits(u), dagger_bernoulli(u, beta), bits(d2), dagger_takeover(d2, tau), gate, bits(act[0]), bits(act[1]), bits(act[2]),
             bits(act[3]));
    }
    return 0;
  }
  fprintf(stderr, "usage: mmx_dagger_selftest draw (seed call t i)... | gate (seed call t i beta tau p[4] e[4])...\n");
  return 2;
}
