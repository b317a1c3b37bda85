// The bounds of time-budgeted launches (csrc/mmx_plan.h rollout_bounds) as a program of its own, built with
// -fsanitize=address,undefined by tests/test_plan_bounds.py.  For every n in 1..600, lanes in 1..8 and fuse in
// 1..32 it checks the rules of a lane's bounds (below; the first violation is printed and the exit status is 1),
// and prints, one JSON object per line:
//   {"kind": "digest", "lanes", "fuse", "plan": an FNV-style hash over the lengths of rollout_plan for n = 1..600,
//    "budgeted": lanes x n cases with lo < hi somewhere}        (the test restates the plan and compares)
//   {"kind": "bounds", "n", "lanes", "fuse", "lane", "len", "lo", "hi"}   for the cases given as "N,LANES,FUSE"
//   {"kind": "override", ...}  the same for "N,LANES,FUSE=PLAN", an MMX_PLAN string
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../mujoco_manip_amd/csrc/mmx_plan.h"

using namespace mmx_host;

static int g_bad = 0;
#define RULE(cond, ...)                \
  do {                                 \
    if (!(cond) && g_bad++ < 20) {     \
      std::fprintf(stderr, "%s: ", #cond); \
      std::fprintf(stderr, __VA_ARGS__);   \
      std::fprintf(stderr, "\n");          \
    }                                  \
  } while (0)

// the rules of one lane's bounds (short calls, fewer than kBudgetMinLaunches = 6 launches, are entirely fixed)
static bool check(const std::vector<int>& len, int n, int nominal, const char* tag) {
  const LaunchBounds B = rollout_bounds(len, nominal, true), F = rollout_bounds(len, nominal, false);
  const size_t K = len.size();
  RULE(B.lo.size() == K && B.hi.size() == K && F.lo.size() == K && F.hi.size() == K, "%s n %d", tag, n);
  bool any = false;
  int c = 0;
  for (size_t j = 0; j < K; j++) {
    c += len[j];
    RULE(B.lo[j] <= c && c <= B.hi[j], "%s n %d launch %zu: lo %d c %d hi %d", tag, n, j, B.lo[j], c, B.hi[j]);
    RULE(B.lo[j] >= 0 && B.hi[j] <= n, "%s n %d launch %zu: lo %d hi %d", tag, n, j, B.lo[j], B.hi[j]);
    RULE(B.hi[j] - B.lo[j] <= nominal, "%s n %d launch %zu: hi - lo %d > len %d", tag, n, j, B.hi[j] - B.lo[j], nominal);
    if (j) RULE(B.lo[j] >= B.lo[j - 1] && B.hi[j] >= B.hi[j - 1], "%s n %d launch %zu: not monotone", tag, n, j);
    RULE(F.lo[j] == c && F.hi[j] == c, "%s n %d launch %zu: the switch off is not fixed", tag, n, j);
    any = any || B.lo[j] < B.hi[j];
  }
  if (K) {
    RULE(B.lo[0] == B.hi[0], "%s n %d: first launch lo %d hi %d", tag, n, B.lo[0], B.hi[0]);
    RULE(B.lo[K - 1] == n && B.hi[K - 1] == n, "%s n %d: last launch lo %d hi %d", tag, n, B.lo[K - 1], B.hi[K - 1]);
  }
  if (K < kBudgetMinLaunches) RULE(!any, "%s n %d: a call of %zu launches is not fixed", tag, n, K);
  return any;
}

static void print_case(const char* kind, int n, int lanes, int fuse, const char* env) {
  const RolloutPlan P = rollout_plan(n, lanes, fuse, false, env);
  const int nominal = rollout_len(n, fuse, false);
  for (int l = 0; l < P.lanes; l++) {
    check(P.len[l], n, nominal, kind);
    const LaunchBounds B = rollout_bounds(P.len[l], nominal, true);
    std::printf("{\"kind\": \"%s\", \"n\": %d, \"lanes\": %d, \"fuse\": %d, \"lane\": %d, \"len\": [", kind, n, lanes, fuse, l);
    for (size_t k = 0; k < P.len[l].size(); k++) std::printf("%s%d", k ? ", " : "", P.len[l][k]);
    std::printf("], \"lo\": [");
    for (size_t k = 0; k < B.lo.size(); k++) std::printf("%s%d", k ? ", " : "", B.lo[k]);
    std::printf("], \"hi\": [");
    for (size_t k = 0; k < B.hi.size(); k++) std::printf("%s%d", k ? ", " : "", B.hi[k]);
    std::printf("]}\n");
  }
}

int main(int argc, char** argv) {
  for (int lanes = 1; lanes <= 8; lanes++)
    for (int fuse = 1; fuse <= 32; fuse++) {
      uint64_t h = 1469598103934665603ull;
      auto mix = [&h](int v) { h = (h ^ uint32_t(v)) * 1099511628211ull; };
      int budgeted = 0;
      for (int n = 1; n <= 600; n++) {
        const RolloutPlan P = rollout_plan(n, lanes, fuse, false, nullptr);
        const int nominal = rollout_len(n, fuse, false);
        mix(P.lanes);
        for (int l = 0; l < P.lanes; l++) {
          mix(-1);
          for (int k : P.len[l]) mix(k);
          budgeted += check(P.len[l], n, nominal, "default");
        }
      }
      std::printf("{\"kind\": \"digest\", \"lanes\": %d, \"fuse\": %d, \"plan\": \"%016llx\", \"budgeted\": %d}\n", lanes, fuse,
                  (unsigned long long)h, budgeted);
    }
  for (int a = 1; a < argc; a++) {
    int n = 0, lanes = 0, fuse = 0;
    if (std::sscanf(argv[a], "%d,%d,%d", &n, &lanes, &fuse) != 3 || n < 0 || lanes < 1 || fuse < 1) {
      std::fprintf(stderr, "usage: %s [N,LANES,FUSE[=PLAN] ...]\n", argv[0]);
      return 2;
    }
    const char* eq = std::strchr(argv[a], '=');
    print_case(eq ? "override" : "bounds", n, lanes, fuse, eq ? eq + 1 : nullptr);
  }
  return g_bad ? 1 : 0;
}
