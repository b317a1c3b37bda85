// Stand-alone host program over csrc/mmx_mppi.h, the closed forms the MPPI kernels run (built by
// tests/test_mppi_host.py with g++ and AddressSanitizer + UndefinedBehaviorSanitizer, run as a child process).
// It prints JSON lines that the test compares with its own restatements:
//   mmx_mppi_selftest philox                      the three known-answer blocks
//   mmx_mppi_selftest draw seed call t i a ...    (groups of five numbers) uniforms and the normal of each element
//   mmx_mppi_selftest update FILE                 the group update of the case in FILE (text: H M K A temperature
//                                                 gamma, box [3][10], nominal, actions, reward, done), every float
//                                                 of the result as its bit pattern
// Exit status 1: the known answers do not come out, or a file cannot be read.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mujoco_manip_amd/csrc/mmx_mppi.h"

static uint32_t bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}
static void print_bits(const char* name, const std::vector<float>& v, const char* end) {
  printf("\"%s\": [", name);
  for (size_t k = 0; k < v.size(); k++) printf("%s%" PRIu32, k ? ", " : "", bits(v[k]));
  printf("]%s", end);
}

static int philox() {
  const uint32_t ctr[3][4] = {{0, 0, 0, 0},
                              {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                              {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}};
  const uint32_t key[3][2] = {{0, 0}, {0xffffffffu, 0xffffffffu}, {0xa4093822u, 0x299f31d0u}};
  const uint32_t want[3][4] = {{0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
                               {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
                               {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};
  int bad = 0;
  for (int c = 0; c < 3; c++) {
    uint32_t out[4];
    mppi_philox4x32_10(ctr[c], key[c], out);
    printf("{\"kind\": \"philox\", \"case\": %d, \"out\": [%" PRIu32 ", %" PRIu32 ", %" PRIu32 ", %" PRIu32 "]}\n", c, out[0],
           out[1], out[2], out[3]);
    bad |= memcmp(out, want[c], sizeof(out)) != 0;
  }
  return bad;
}

static int draw(int argc, char** argv) {
  for (int k = 2; k + 4 < argc; k += 5) {
    const uint64_t seed = strtoull(argv[k], nullptr, 0), call = strtoull(argv[k + 1], nullptr, 0);
    const uint32_t t = (uint32_t)strtoul(argv[k + 2], nullptr, 0), i = (uint32_t)strtoul(argv[k + 3], nullptr, 0),
                   a = (uint32_t)strtoul(argv[k + 4], nullptr, 0);
    float u1, u2;
    mppi_draw_uniforms((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)call, (uint32_t)(call >> 32), t, i, a, &u1, &u2);
    const float z = mppi_draw((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)call, (uint32_t)(call >> 32), t, i, a);
    printf("{\"kind\": \"draw\", \"seed\": %" PRIu64 ", \"call\": %" PRIu64 ", \"t\": %u, \"i\": %u, \"a\": %u, \"u1\": %.17g, "
           "\"u2\": %.17g, \"z\": %.9g}\n", seed, call, t, i, a, (double)u1, (double)u2, (double)z);
  }
  return 0;
}

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n, const char* fmt) {
  v.resize(n);
  for (size_t k = 0; k < n; k++)
    if (fscanf(f, fmt, &v[k]) != 1) return false;
  return true;
}

static int update(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return 1;
  MppiParams P{};
  float temperature = 0.f;
  std::vector<float> box, nominal, actions, reward;
  std::vector<int> done;
  bool ok = fscanf(f, "%d %d %d %d %f %f", &P.H, &P.M, &P.K, &P.A, &temperature, &P.gamma) == 6;
  ok = ok && P.H >= 1 && P.H <= MPPI_MAX_HORIZON && P.A >= 1 && P.A <= MPPI_MAX_ADIM && P.M >= 1 && P.K >= 1;
  const size_t H = (size_t)P.H, M = (size_t)P.M, N = M * (size_t)P.K, A = (size_t)P.A;
  ok = ok && read_n(f, box, 3 * MPPI_MAX_ADIM, "%f") && read_n(f, nominal, H * M * A, "%f") &&
       read_n(f, actions, H * N * A, "%f") && read_n(f, reward, H * N, "%f") && read_n(f, done, H * N * 3, "%d");
  fclose(f);
  if (!ok) return 1;
  P.inv_lambda = temperature > 0.f ? 1.f / temperature : 0.f;
  std::vector<float> returns(N), weights(N), out(M * A);
  std::vector<int> best(M);
  MppiBufs B{nominal.data(), nullptr, actions.data(), reward.data(), done.data(), returns.data(), weights.data(), best.data()};
  for (int m = 0; m < P.M; m++) mppi_group_update_ref(P, B, box.data(), m, out.data());
  std::vector<float> finite(N);
  for (size_t i = 0; i < N; i++) finite[i] = mppi_finite(returns[i]) ? 1.f : 0.f;
  printf("{\"kind\": \"update\", ");
  print_bits("returns", returns, ", ");
  print_bits("weights", weights, ", ");
  print_bits("nominal", nominal, ", ");
  print_bits("action_out", out, ", ");
  print_bits("finite", finite, ", ");
  printf("\"best\": [");
  for (size_t m = 0; m < M; m++) printf("%s%d", m ? ", " : "", best[m]);
  printf("]}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "philox")) return philox();
  if (argc >= 2 && !strcmp(argv[1], "draw")) return draw(argc, argv);
  if (argc == 3 && !strcmp(argv[1], "update")) return update(argv[2]);
  fprintf(stderr, "usage: mmx_mppi_selftest philox | draw (seed call t i a)... | update FILE\n");
  return 2;
}
