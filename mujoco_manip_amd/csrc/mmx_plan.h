// Launch plan of an n-step rollout.  Host code only, no HIP: tests/host/mmx_host_selftest.cpp prints the
// plans under the sanitizers and tests/test_host_selftest.py checks them; tests/host/mmx_plan_bounds_selftest.cpp
// and tests/test_plan_bounds.py do the same for the bounds of the time-budgeted launches (rollout_bounds).
//
// Without cameras a launch runs `len` consecutive env steps of its lane's envs, len = min(fuse, ceil(n / 4));
// lane l of L starts with a launch of l * len / L steps (none for lane 0), then launches of len, then the
// remainder, so the lanes' launch boundaries are spread over the launch period instead of falling together.
// Every launch ends with a drain (its slowest workgroups finish while its slots empty); the other lanes fill
// the slots it frees as long as they are not draining at the same time.  Measured on the driver's 20-step windows
// (tools/sweep_env.py, profiles/r06_sweep_driver_plans.json): equal 3-step launches, all lanes in step,
// 2.72 M env steps/s; the staggered 5-step plan 2.87 M (+5.4 %); staggered 3-, 4-, 6-, 7-, 10-step
// plans and 1-step final launches between them; 512-step windows +0.5 % (16-step launches offset by 4).
// With cameras every step is rendered: one step per launch, one lane.
#ifndef MMX_PLAN_H
#define MMX_PLAN_H
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

namespace mmx_host {

// Multi-step rollouts split the envs into lanes, independent ranges each stepped on its own stream
constexpr int kMaxLanes = 8;

inline int rollout_len(int n, int fuse, bool cameras) {
  return cameras ? 1 : std::max(1, std::min(fuse, n / 4 + (n % 4 != 0)));
}
// lanes of a rollout: with cameras one (every step ends in the render over all envs, and one launch
// orders all envs longest-first: C5 +2.0 % over 4 lanes)
inline int rollout_lanes(int lanes, bool cameras) { return cameras ? 1 : lanes; }

// Launch lengths of every lane for an n-step rollout (above): `lanes` of them (one for a single step),
// `rounds` = the most launches any lane makes.  plan_env (the MMX_PLAN variable, or null) =
// "a,b,...[;c,d,...]" per lane (the last list repeats for the lanes after it) overrides a lane's lengths
// for experiments when they sum to n.
struct RolloutPlan {
  int lanes = 0;
  size_t rounds = 0;
  std::vector<int> len[kMaxLanes];
};
inline RolloutPlan rollout_plan(int n, int lanes, int fuse, bool cameras, const char* plan_env) {
  RolloutPlan P;
  const int L = std::max(1, std::min(rollout_lanes(lanes, cameras), kMaxLanes));
  P.lanes = n > 1 ? L : 1;
  for (int lane = 0; lane < P.lanes; lane++) {
    std::vector<int>& v = P.len[lane];
    if (plan_env) {
      std::string all(plan_env), mine;
      size_t pos = 0;
      for (int l = 0;; l++) {
        const size_t sc = all.find(';', pos);
        mine = all.substr(pos, sc == std::string::npos ? std::string::npos : sc - pos);
        if (l == lane || sc == std::string::npos) break;
        pos = sc + 1;
      }
      int sum = 0;
      for (size_t a = 0; a < mine.size();) {
        const long k = std::strtol(mine.c_str() + a, nullptr, 10);
        if (k <= 0) break;
        if (k > n - sum) {  // past n: not this rollout's plan (and the sum cannot overflow)
          sum = -1;
          break;
        }
        v.push_back(static_cast<int>(k));
        sum += static_cast<int>(k);
        const size_t c = mine.find(',', a);
        if (c == std::string::npos) break;
        a = c + 1;
      }
      if (sum != n) v.clear();
    }
    if (v.empty() && n > 0) {
      const int len = rollout_len(n, fuse, cameras);
      int rem = n;
      const int first = std::min(rem, lane * len / L);
      if (first > 0) {
        v.push_back(first);
        rem -= first;
      }
      for (; rem > 0; rem -= std::min(rem, len)) v.push_back(std::min(rem, len));
    }
    P.rounds = std::max(P.rounds, v.size());
  }
  return P;
}

// Time-budgeted launches (mmx_env_step_budget_kernel): the bounds on an env's step count of the call after each
// launch of one lane, from the lane's lengths `len` (a row of rollout_plan), their sum n and the plan's
// nominal length (rollout_len).  With c_j the count after launch j in the fixed plan and s_j a spread,
//   lo_j = max(0, c_j - s_j),  hi_j = min(n, c_j + s_j):
// a launch's workgroups stop by the clock anywhere in [lo_j, hi_j], so the lane's next launch finds slots
// freed together, and no env is ever more than s_j steps off the plan.  s_j is nominal / 2 in the middle of
// a call; 0 at the first launch (no step-time estimate yet) and at the last (every env ends at n); it halves
// per launch towards the end (nominal / 2, / 4, / 8, 0), so the call's one full drain is a short one; and it
// changes by at most len_j from one launch to the next, which keeps both sequences non-decreasing under any
// MMX_PLAN.  Fixed (lo_j = hi_j = c_j) when `budget` is off or the lane makes fewer than 6 launches (the first,
// one at the full spread, the three of the taper, the last): every call of fewer than 4 launches, and the
// 20-step windows of the training driver (4 or 5 launches of 5 steps), whose measured plan stays as it is.
struct LaunchBounds {
  std::vector<int> lo, hi;
};
constexpr size_t kBudgetMinLaunches = 6;
inline LaunchBounds rollout_bounds(const std::vector<int>& len, int nominal, bool budget) {
  LaunchBounds B;
  const size_t K = len.size();
  std::vector<int> c(K), s(K, 0);
  int n = 0;
  for (size_t j = 0; j < K; j++) c[j] = n += len[j];
  if (budget && K >= kBudgetMinLaunches) {
    const int full = std::max(0, nominal / 2);
    for (size_t j = 1; j + 1 < K; j++) {
      const size_t d = K - 1 - j;  // launches after this one
      s[j] = std::min(d >= 3 ? full : full >> (3 - d), s[j - 1] + len[j]);
    }
    for (size_t j = K - 1; j-- > 0;) s[j] = std::min(s[j], s[j + 1] + len[j + 1]);
  }
  for (size_t j = 0; j < K; j++) {
    B.lo.push_back(std::max(0, c[j] - s[j]));
    B.hi.push_back(std::min(n, c[j] + s[j]));
  }
  return B;
}

}  // namespace mmx_host

#endif
