// The library's host-only code (csrc/mmx_seed.h, csrc/mmx_plan.h) as a program of its own, built with
// -fsanitize=address,undefined by tests/test_host_selftest.py, which checks what it prints (one JSON object
// per line) against numpy and the plan's rules.  Arguments: "N=PLAN" each, a MMX_PLAN string for an N-step
// rollout on 4 lanes without cameras (PLAN may be empty).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../mujoco_manip_amd/csrc/mmx_plan.h"
#include "../../mujoco_manip_amd/csrc/mmx_seed.h"

using namespace mmx_host;

static void print_plan(int arg, int n, int lanes, int fuse, int cameras, const char* env) {
  const RolloutPlan P = rollout_plan(n, lanes, fuse, cameras != 0, env);
  std::printf("{\"kind\": \"plan\", \"arg\": %d, \"n\": %d, \"lanes\": %d, \"fuse\": %d, \"cameras\": %d, \"rounds\": %zu, \"len\": [",
              arg, n, lanes, fuse, cameras, P.rounds);
  for (int l = 0; l < P.lanes; l++) {
    std::printf("%s[", l ? ", " : "");
    for (size_t k = 0; k < P.len[l].size(); k++) std::printf("%s%d", k ? ", " : "", P.len[l][k]);
    std::printf("]");
  }
  std::printf("]}\n");
}

int main(int argc, char** argv) {
  for (uint64_t seed : {uint64_t(0), uint64_t(42), (uint64_t(1) << 40) + 3, ~uint64_t(0)}) {
    uint64_t st[4];
    pcg64_seed(seed, st);
    unsigned long long row[4];
    pcg64_seed_row(row, seed);
    for (int k = 0; k < 4; k++)
      if (row[k] != st[k]) return 1;
    std::printf("{\"kind\": \"pcg64\", \"seed\": %" PRIu64 ", \"state\": [%" PRIu64 ", %" PRIu64 "], \"inc\": [%" PRIu64 ", %" PRIu64 "]}\n",
                seed, st[0], st[1], st[2], st[3]);
  }
  const struct {
    uint64_t root;
    int count;
  } spawns[] = {{42, 64}, {(uint64_t(1) << 40) + 3, 8}};
  for (const auto& s : spawns)
    for (int i = 0; i < s.count; i++)
      std::printf("{\"kind\": \"spawn\", \"root\": %" PRIu64 ", \"index\": %d, \"value\": %" PRIu32 "}\n", s.root, i,
                  episode_seed(s.root, i));
  const int cases[][4] = {{0, 3, 32, 0}, {1, 3, 32, 0}, {2, 3, 32, 0}, {20, 4, 32, 0},
                          {43, 1, 7, 0}, {43, 3, 32, 0}, {512, 3, 32, 0}, {43, 3, 32, 1}};
  for (const auto& c : cases) print_plan(-1, c[0], c[1], c[2], c[3], nullptr);
  for (int a = 1; a < argc; a++) {
    const char* eq = std::strchr(argv[a], '=');
    if (!eq) {
      std::fprintf(stderr, "usage: %s [N=PLAN ...]\n", argv[0]);
      return 2;
    }
    print_plan(a - 1, std::atoi(argv[a]), 4, 32, 0, eq + 1);
  }
  return 0;
}
