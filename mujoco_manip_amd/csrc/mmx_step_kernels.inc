// Part 8 of mmx_step.inc, its last (an ordered fragment, included there and nowhere else): the end of an env
// step (step_end), the out-of-line substep / step_begin / step_finish, the profile build's stamps, the fused
// step loop, stated once per wave (MMX_ENV_WAVE_STEPS, MMX_HELPER_WAVE_STEPS) with the kernel entry
// (MMX_STEP_KERNEL_ENTRY), the five fused step kernels built from them and the one-substep kernel, and their
// launchers.  Relies on every part before it: the record g_E and the scratch map (lds), kinematics_wave /
// dynamics_wave (dynamics), the collide_* passes (collision), ik_wave and mj_step_wave (integrate), EPI / EPF,
// the task layer and load_env / store_env / store_obs (task), on mmx_policy.h for policy_act and on mmx_dagger.h
// for dagger_begin.
// ============================================================================ kernels
// One env per 64-lane workgroup.  mmx_env_step_kernel (below) is the product path: a whole gym
// step per launch.  mmx_substep_kernel runs ONE substep per launch (the physics-level parity
// harness, mmx_physics_step, and a gym step split over 16 launches when mode has SS_GYM): the
// first launch decodes the action (or runs the FSM expert's plan(16)), the last runs the
// mj_forward position stage, reward, observation and autoreset (gym_env.py:536-581).
enum { SS_FIRST = 1, SS_LAST = 2, SS_EXPERT = 4, SS_IK = 8, SS_GYM = 16 };

DEV void fold_flags(const MMXState& S, int i, const EnvSh& E) {  // lane 0
  if (E.flags & SHF_CON_OVF) EPI(EPI_ERROR) |= ERR_CON_OVERFLOW;
  if (E.flags & SHF_EFC_OVF) EPI(EPI_ERROR) |= ERR_EFC_OVERFLOW;
  if (E.flags & SHF_NAN) EPI(EPI_ERROR) |= ERR_NAN;
}

// reward, termination and info of the current state (gym_env.py:562-573): writes the reward and
// the reward components, adds the reward to the episode return; lane 0
DEV void reward_outputs(const MMXState& S, int i, EnvSh& E, bool robot_obstacle, int& terminated, int& succ_flag) {
  int success = 0;
  const float r = reward_lane0(S, i, E, robot_obstacle, success);
  float* rc = S.reward_components + (size_t)i * 6;
  if (S.reward_type == 2) {
    terminated = (r < 0.f) || success;
    succ_flag = success && r >= 0.f;
    float sum = 0.f;
    for (int k = 0; k < 5; k++) {
      const float h = EPF(EPF_HWM + k) / 5.f;
      rc[1 + k] = h;
      sum += h;
    }
    rc[0] = sum;
  } else {
    terminated = success;
    succ_flag = success;
    for (int k = 0; k < 6; k++) rc[k] = 0.f;
  }
  S.reward[i] = r;
  EPF(EPF_EP_RETURN) += r;
}

// end of PickPlaceGymEnv.step: position stage, staged-penalty contact scan, reward, obs, autoreset
DEV void step_end(const MMXState& S, int i, EnvSh& E) {
  float* stats = E.stats;
  CLK_DECL;
  // mj_forward position stage (gym_env.py:560): kinematics + contacts for the staged penalty
  if (LANE == 0) {
    EPI(EPI_NCON) = E.ncon;
    EPI(EPI_NEFC) = E.nefc_mj;
  }
  kinematics_wave(E);
  if (S.reward_type == 2) collide_wave(E, true);
  if (LANE == 0) {
    EPI(EPI_STEP) += 1;
    int terminated, succ_flag;
    reward_outputs(S, i, E, (E.flags & SHF_ROBOT_OBST) != 0, terminated, succ_flag);
    const int truncated = EPI(EPI_STEP) >= S.max_episode_steps;
    S.done[3 * (size_t)i] = terminated;
    S.done[3 * (size_t)i + 1] = truncated;
    S.done[3 * (size_t)i + 2] = succ_flag;
    fold_flags(S, i, E);
    obs_lane0(S, i, E);
    // the FSM state only moves when the expert plans (mmx_expert_plan, or inside the rollout's
    // step launch), so host-action steps never see DONE: expert_plan + step autoresets exactly like
    // the fused rollout
    const bool fsm_done = EPI(EPI_FSM_STATE) == 10;
    const bool err = (EPI(EPI_ERROR) & ERR_NAN) != 0;
    if (S.autoreset && (terminated || truncated || err || fsm_done)) {
      if (err) {  // a diverged env ends its episode as truncated, not as a silent reset
        S.done[3 * (size_t)i + 1] = 1;
        S.done[3 * (size_t)i + 2] = 0;
        EPI(EPI_NERROR) += 1;
      } else {
        // an episode ended by the expert's FSM alone (no termination, no time limit) is reported as
        // truncated, so every autoreset carries a done flag (ended outside the MDP, like a time limit)
        if (!terminated) S.done[3 * (size_t)i + 1] = 1;
        EPI(EPI_NSUCCESS) += succ_flag;
        EPI(EPI_NPLACED) += in_target_bin(S, i, E) ? 1 : 0;
      }
      EPI(EPI_ERROR) = 0;
      reset_lane0(S, i, E, -1);
    }
    CLK(stats, STAT_T_END);
  }
  store_obs(S, i, E);
}

// One substep = IK + mj_step, kept out of line: nothing is hoisted across the 16 iterations of
// the env-step loop (hoisted invariants would pin registers for the whole kernel and serialise
// the phases' LDS loads).  The call costs no register save: substep, step_begin and step_finish
// have local linkage after the device link's internalisation, do not recurse and never have their
// address taken, so the AMDGPU backend compiles them without callee-saved registers -- provided no
// call site of theirs carries the IR `tail` marker, which the optimiser stamps on any call that does
// not touch the caller's stack, and which alone switches that path off.  MMX_NO_TAIL_MARK on the
// caller keeps the marker away; every function that calls one of the three needs it (one marked site
// brings the saves back: at the 168-VGPR cap 64 VGPRs stored and reloaded per call, 16 KB per wave,
// 16 calls per env step, which was 178 KB of HBM writes per env step).  The caller instead keeps
// its own few live values (env index, loop counters, pointers) in SGPRs / reloads them after a call.
#define MMX_NO_TAIL_MARK __attribute__((disable_tail_calls))
//
// (Measured and removed: splitting one env over two waves, wave 1 running the collision prune and
// the plane / box-box pairs beside wave 0's dynamics and GJK/EPA: register-bound at 4 workgroups per
// CU, 1.11 M env steps/s against 1.21 M for one wave at 5 / CU, before the LDS shrink to 8 / CU.)
__device__ __attribute__((noinline)) void substep(int max_iter, float tol, float* con_dst) {
  EnvSh& E = g_E;
  float* stats = E.stats;
  CLK_DECL;
#if !MMX_STEP_HELPER  // (the helper wave's, beside the kinematics: mj_step_wave)
  ik_wave(E);  // IK on the kinematics left by the previous position stage
#endif
  CLK(stats, STAT_T_IK);
  mj_step_wave(max_iter, tol, E, con_dst);
}

// Lane 0 takes the env step's action (step_begin, and mmx_substep_kernel's first launch of a gym step): the FSM
// expert's plan(16) or the env's row of `action`, into the scratch slot SCR_ACT (E.J is free before the
// substeps), then the decode into the record's target.
DEV void take_action_lane0(const MMXState& S, int i, EnvSh& E, const float* action, int adim, int expert) {
  float* act = scr_of(E) + SCR_ACT;
  if (expert) expert_plan(S, i, obj_pos(E, EPI(EPI_OBJ)), hand_pos(E), MMX_NSUBSTEP, act);
  else
    for (int k = 0; k < adim && k < 12; k++) act[k] = action[(size_t)i * adim + k];
  decode_lane0(S, i, E, act);
}
// The step's prologue (record load, FSM plan, action decode) and epilogue (position stage, reward,
// observation, autoreset, record store) are out of line like the substep: inlined into the fused
// step loop they kept ~280 VGPRs of hoisted values live across iterations (scratch spills).  Like
// the substep they save no registers for their caller (MMX_NO_TAIL_MARK on the kernel).
__device__ __attribute__((noinline)) void step_begin(const MMXState& S, int i, const float* action, int adim,
                                                     int expert) {
  EnvSh& E = g_E;
  load_env(S, i, E);
  if (LANE == 0) take_action_lane0(S, i, E, action, adim, expert);
  SYNC();
}
__device__ __attribute__((noinline)) void step_finish(const MMXState& S, int i) {
  EnvSh& E = g_E;
  step_end(S, i, E);
  store_env(S, i, E);
}
#ifdef MMX_PHASE_CLOCK
// Diagnostic build only: per FSM state of the env step (the state the step's action was planned
// in), the sums over env steps of the shader cycles of each phase (STAT_T_IK .. STAT_T_END), of
// the whole step, of the solver iterations / MuJoCo rows / contacts, the whole step's constant-rate
// wall clock (100 MHz ticks: the slot time an env step holds, and with FSMP_STEP the shader clock) and
// the env-step count (tools/gpu_probe.py fsm_profile).  Lane 0 of each env adds with global atomics.
enum { FSMP_PHASES = STAT_T_AUX3 - STAT_T_IK + 1, FSMP_STEP = FSMP_PHASES, FSMP_ITER, FSMP_NEFC, FSMP_NCON,
       FSMP_RT, FSMP_COUNT, FSMP_N };
// (one copy per translation unit: mmx_kernels.hip reads out its own, the 128-row kernels', in
// mmx_fsm_profile; the 192-row object's stays private to it)
static __device__ double g_fsm_prof[11 * FSMP_N];
// the profile's four stamps of an env step, for the step kernels' loops (below)
#define FSMP_STEP_START const unsigned long long rt_step = wall_clock64() /* (the record load and the plan included) */
#define FSMP_SUBSTEPS_START                                                         \
  float snap[FSMP_N];                                                               \
  const int fsm = EPI(EPI_FSM_STATE);                                               \
  const unsigned long long t_step = clk_now();                                      \
  if (LANE == 0) {                                                                  \
    for (int j = 0; j < FSMP_PHASES; j++) snap[j] = g_E.stats[STAT_T_IK + j];       \
    snap[FSMP_ITER] = g_E.stats[STAT_SOLVER_ITER];                                  \
    snap[FSMP_NEFC] = g_E.stats[STAT_NEFC];                                         \
    snap[FSMP_NCON] = g_E.stats[STAT_NCON];                                         \
  }
/* (read before step_finish stores the record: an autoreset does not clear stats) */
#define FSMP_SUBSTEPS_END                                                                                           \
  if (LANE == 0) {                                                                                                  \
    double* g = g_fsm_prof + FSMP_N * min(max(fsm, 0), 10);                                                         \
    for (int j = 0; j < FSMP_PHASES; j++) atomicAdd(g + j, (double)(g_E.stats[STAT_T_IK + j] - snap[j]));           \
    atomicAdd(g + FSMP_ITER, (double)(g_E.stats[STAT_SOLVER_ITER] - snap[FSMP_ITER]));                              \
    atomicAdd(g + FSMP_NEFC, (double)(g_E.stats[STAT_NEFC] - snap[FSMP_NEFC]));                                     \
    atomicAdd(g + FSMP_NCON, (double)(g_E.stats[STAT_NCON] - snap[FSMP_NCON]));                                     \
  }
#define FSMP_STEP_END                                                                                               \
  if (LANE == 0) {                                                                                                  \
    double* g = g_fsm_prof + FSMP_N * min(max(fsm, 0), 10);                                                         \
    atomicAdd(g + STAT_T_END - STAT_T_IK, (double)(g_E.stats[STAT_T_END] - snap[STAT_T_END - STAT_T_IK]));          \
    atomicAdd(g + FSMP_STEP, (double)(clk_now() - t_step));                                                         \
    atomicAdd(g + FSMP_RT, (double)(wall_clock64() - rt_step));                                                     \
    atomicAdd(g + FSMP_COUNT, 1.0);                                                                                 \
  }
#else
#define FSMP_STEP_START
#define FSMP_SUBSTEPS_START
#define FSMP_SUBSTEPS_END
#define FSMP_STEP_END
#endif
// (the stamps of a kernel without a per-phase profile, in every build: MMX_ENV_WAVE_STEPS's `stamps` argument)
#define NOFSMP_STEP_START
#define NOFSMP_SUBSTEPS_START
#define NOFSMP_SUBSTEPS_END
#define NOFSMP_STEP_END

// waves per SIMD the step kernel's register allocation is made for: 3 for the 128-row layout (168
// VGPRs: twelve envs per CU); 2 for the 192-row layout, the one for batches that leave CU slots empty
// (C2's 1024 envs are four per CU, each an env wave and its helper wave: eight waves per CU, 248 VGPRs;
// C2 1.29 -> 1.52 M, profiles/r06_ab_c2_helper.json; without the helper it ran one wave per SIMD)
#ifndef MMX_STEP_WAVES
#define MMX_STEP_WAVES (MMX_LDSEFC == 128 ? 3 : (MMX_STEP_HELPER ? 2 : 1))
#endif
#define MMX_STEP_THREADS (MMX_STEP_HELPER ? 128 : 64)  // the env's wave (+ the helper wave)
#ifndef MMX_STEP_SUFFIX
#define MMX_STEP_SUFFIX
#endif
#define MMX_CAT2_(a, b) a##b
#define MMX_CAT_(a, b) MMX_CAT2_(a, b)
#define MMX_STEP_SYM(name) MMX_CAT_(name, MMX_STEP_SUFFIX)
// What stands in front of a fused step kernel's name: the launch bounds, the occupancy the registers are
// allocated for, and MMX_NO_TAIL_MARK, which every caller of substep / step_begin / step_finish needs (see
// above it: one call site without it brings the callee-saved register saves back into all three).
#define MMX_STEP_KERNEL                                          \
  extern "C" __global__ void __launch_bounds__(MMX_STEP_THREADS) \
      __attribute__((amdgpu_waves_per_eu(MMX_STEP_WAVES, MMX_STEP_WAVES))) MMX_NO_TAIL_MARK

#if MMX_STEP_HELPER
// The helper wave's side of `nsteps` env steps of a fused step kernel (192 rows: threads 64..127), stated once
// for mmx_env_step_kernel, mmx_env_traj_kernel, mmx_env_policy_kernel and mmx_env_dagger_kernel, which take it
// through their entry (MMX_STEP_KERNEL_ENTRY).  It crosses exactly the workgroup barriers of the env wave's step
// loop (MMX_ENV_WAVE_STEPS), no path of either wave skipping one: between two steps the fence and the barrier
// behind the record stores, then the barrier after step_begin's record load, then per substep C, K, A, P, Q, the table in
// mj_step_wave (mmx_step_integrate.inc), with the helper's work between them: the IK in C..K, the dynamics in
// A..P, the GJK / EPA pairs in P..Q.  What a kernel's env wave adds around step_begin and step_finish --
// policy_act before, traj_record after, dagger_begin in step_begin's place -- holds no workgroup barrier, so the
// helper has nothing to mirror for it: it waits at the record-load barrier meanwhile.  mmx_substep_kernel
// follows the same sequence for its one substep.
// A macro, not a function: the loop as one force-inlined DEV function keeps every instruction count and still
// changes the register allocation of all three 192-row kernels (tried twice, and once more when this macro was
// written: the listings first differ in a v_cndmask_b32_e64 v64 that becomes v7), while these tokens pasted
// into each kernel leave the listings instruction for instruction what three written-out copies gave
// (tools/isa_same.py).  Do not convert it.
#define MMX_HELPER_WAVE_STEPS(nsteps)                                                                        \
  for (int k = 0; k < (nsteps); k++) {                                                                       \
    if (k) { /* the env wave's record stores of the previous step */                                         \
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");                                                 \
      XSYNC();                                                                                               \
    }                                                                                                        \
    XSYNC(); /* step_begin's record load */                                                                  \
    for (int sub = 0; sub < MMX_NSUBSTEP; sub++) {                                                           \
      __syncthreads(); DELAY_HELPER(); ik_wave(g_E);       /* C, the IK */                                   \
      __syncthreads(); /* K: the IK has read the kinematics cache; the env wave may overwrite it */          \
      __syncthreads(); DELAY_HELPER(); dynamics_wave(g_E); /* A, the dynamics */                             \
      __syncthreads(); collide_pairs(g_E, false, 2);       /* P, the GJK / EPA pairs */                      \
      __syncthreads();                                     /* Q */                                           \
    }                                                                                                        \
  }
#define MMX_HELPER_WAVE_BRANCH                                                                               \
  if (threadIdx.x >= 64) { /* the helper wave: the same workgroup barriers as the env's wave */              \
    MMX_HELPER_WAVE_STEPS(nsteps)                                                                            \
    return;                                                                                                  \
  }
#else
#define MMX_HELPER_WAVE_BRANCH
#endif

// The env wave's side of the same loop, stated once for all five fused kernels: env steps k = 0 .. nsteps - 1 of
// env i of S.  What the loop guarantees, whatever a kernel hangs on it:
//  - each iteration is exactly one single-step launch's body -- the record loaded (`begin`: step_begin, or
//    dagger_begin in its place, behind whatever computes the action), the 16 out-of-line substeps, the record and
//    the outputs stored (step_finish) -- and between two iterations the previous step's record and observation
//    stores complete before the next one reads them (the seam: fence and workgroup barrier).  So a fused launch
//    is bit for bit the same number of single-step launches, however the steps fall into launches;
//  - the workgroup barriers are the seam's, the record-load barrier behind `begin` and those of the substeps, and
//    no others: `begin` and `after` are a kernel's own statements (they may use k, and what `begin` declares is
//    in scope for `after`) and must hold NO workgroup barrier, because the helper wave of the 192-row layout
//    crosses exactly the barriers stated here (MMX_HELPER_WAVE_STEPS) and a barrier on one side only hangs it.
// `nsteps` is read again at every test, so `after` may raise it (the budgeted kernel's open-ended count).
// `stamps` is FSMP for the profile build's per-phase stamps around the step and its substeps, NOFSMP for none.
// A macro for the reason given at MMX_HELPER_WAVE_STEPS: pasted tokens leave the five kernels' listings what the
// written-out copies gave (tools/isa_same.py, profiles/r22_isa_same.json).  Do not convert it.
#define MMX_ENV_WAVE_STEPS(nsteps, stamps, begin, after)                                                     \
  for (int k = 0; k < (nsteps); k++) {                                                                       \
    if (k) { /* the seam */                                                                                  \
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");                                                 \
      XSYNC();                                                                                               \
    }                                                                                                        \
    stamps##_STEP_START;                                                                                     \
    begin;                                                                                                   \
    XSYNC(); /* the record load */                                                                           \
    stamps##_SUBSTEPS_START                                                                                  \
    for (int sub = 0; sub < MMX_NSUBSTEP; sub++)                                                             \
      substep(S.solver_max_iter, S.solver_tol, sub == MMX_NSUBSTEP - 1 ? contacts_dst(S, i) : nullptr);      \
    stamps##_SUBSTEPS_END                                                                                    \
    step_finish(S, i);                                                                                       \
    stamps##_STEP_END                                                                                        \
    after;                                                                                                   \
  }
// A fused kernel's entry, from its arguments S, base, order and (192 rows) nsteps: the env index i -- order
// (optional) lists the launch's envs in dispatch order, the grasp-carrying ones first (mmx_order_kernel) -- the
// bounds test, and the helper wave's whole part in the kernel.
#define MMX_STEP_KERNEL_ENTRY                                  \
  const int i = order ? order[blockIdx.x] : base + blockIdx.x; \
  if (i >= S.N) return;                                        \
  MMX_HELPER_WAVE_BRANCH

// The whole PickPlaceGymEnv.step in ONE launch (product path): the 16 substeps loop inside the workgroup, so
// per-env cost variation averages out over the step instead of stretching 16 separate launch tails (measured:
// one launch per substep ran 40 % slower).  With the on-device FSM expert (expert = 1) a launch may also run
// `nsteps` consecutive env steps of its env, minus nsteps - 1 launch tails.  The per-phase profile's kernel.
MMX_STEP_KERNEL MMX_STEP_SYM(mmx_env_step_kernel)(MMXState S, const float* action, int adim, int expert, int base, int nsteps,
                                                  const int* order) {
  MMX_STEP_KERNEL_ENTRY
  MMX_ENV_WAVE_STEPS(nsteps, FSMP, step_begin(S, i, action, adim, expert), )
}

#if !MMX_STEP_HELPER
// The launch's clock for the budget: the constant-rate counter (100 MHz) -- or, in the test build
// libmmx_synth.so (MMX_BUDGET_SYNTH), a cost of 1 + env % 3 "ticks" per env step, k = the steps of this
// launch so far: uneven progress that does not depend on the machine (tests/test_step_budget.py).
DEV unsigned long long budget_now(int k, int i) {
#ifdef MMX_BUDGET_SYNTH
  return (unsigned long long)k * (unsigned long long)(1 + i % 3);
#else
  return wall_clock64();
#endif
}
// mmx_env_step_kernel's expert step loop with a time budget in place of a step count (mmx_rollout_expert
// on this, the one-wave layout, without cameras; MMXBudget in mmx_state.h).  The envs of a launch cost
// 1.45 M to 2.5 M cycles a step by FSM phase, so after equal counts they end milliseconds apart and the
// slots of the early ones stay empty until the lane's next launch; after equal times they end within a step
// of each other, the cheap envs a few steps ahead of the plan and the dear ones behind it, every env
// inside [lo, hi].  The test is made once per env step, after step_finish, from scalar values (the count, the
// bounds, the clock), so it is the same for the whole wave;
// lane 0 then writes the env's count back and adds the workgroup's steps and ticks to the launch's sums, from
// which the lane's next launch (same stream: ordered after this one) takes its ticks per step.
MMX_STEP_KERNEL mmx_env_step_budget_kernel(MMXState S, MMXBudget B, const float* action, int adim, int base,
                                           const int* order) {
  MMX_STEP_KERNEL_ENTRY
  const int first = __builtin_amdgcn_readfirstlane(B.done[i]);
  const unsigned long long t0 = budget_now(0, i);
  unsigned long long budget = 0;
  unsigned long long* const sum = B.acc + 2 * (B.round % 3);
  if (blockIdx.x == 0 && LANE == 0) {  // the next launch's pair (MMXBudget: nobody reads or adds to it now)
    unsigned long long* const next = B.acc + 2 * ((B.round + 1) % 3);
    next[0] = next[1] = 0;
  }
  if (B.lo < B.hi) {
    const unsigned long long* const last = B.acc + 2 * ((B.round + 2) % 3);
    const unsigned long long steps = last[0], ticks = last[1];
    if (steps) budget = (unsigned long long)((float)B.nominal * ((float)ticks / (float)steps));
  }
  // the count is open at the end: at least up to lo, then a step at a time while the clock and hi allow
  const int most = B.hi - first;
  int nsteps = max(B.lo - first, most > 0 && budget > 0 ? 1 : 0);
  MMX_ENV_WAVE_STEPS(nsteps, FSMP, step_begin(S, i, action, adim, 1),
                     if (k + 1 == nsteps) nsteps += __builtin_amdgcn_readfirstlane(nsteps < most && budget_now(nsteps, i) - t0 < budget))
  if (LANE == 0) {
    B.done[i] = first + nsteps;
    if (B.log) B.log[i] = first + nsteps;
    if (nsteps > 0) {
      atomicAdd(sum, (unsigned long long)nsteps);
      atomicAdd(sum + 1, budget_now(nsteps, i) - t0);
    }
  }
}
#endif

// The env's outputs after an env step, into slice `row` = step * N + env of the trajectory arrays.
// Runs on the env's wave right after step_finish and needs no barrier of its own: the observation,
// positions, velocities and target are read from the LDS record behind the SYNC() of store_obs /
// store_env, by the lanes that stored them to the sim's buffers (after an autoreset: the new episode's);
// reward, flags, components and the integer episode record were written to the sim's buffers by lane 0,
// which reads its own stores back.  The helper wave (192 rows) has nothing to mirror.
DEV void traj_record(const MMXState& S, const MMXTraj& R, int i, size_t row) {
  const EnvSh& E = g_E;
  if (R.obs)
    for (int k = LANE; k < MMX_NOBS; k += WG) R.obs[row * MMX_NOBS + k] = obs_of(E)[k];
  if (R.qpos && LANE < 30) R.qpos[row * 30 + LANE] = E.qpos[LANE];
  if (R.qvel && LANE < 27) R.qvel[row * 27 + LANE] = E.qvel[LANE];
  if (R.target && LANE < 4) R.target[row * 4 + LANE] = E.target[LANE];
  if (LANE == 0) {
    if (R.reward) R.reward[row] = S.reward[i];
    if (R.done)
      for (int k = 0; k < 3; k++) R.done[row * 3 + k] = S.done[3 * (size_t)i + k];
    if (R.reward_components)
      for (int k = 0; k < 6; k++) R.reward_components[row * 6 + k] = S.reward_components[(size_t)i * 6 + k];
    if (R.epi)
      for (int k = 0; k < EPI_N; k++) R.epi[row * EPI_N + k] = EPI(k);
  }
}

// mmx_env_step_kernel's step loop with an action row per step and a per-step record (mmx_rollout_actions,
// mmx_rollout_expert_record): step k of the launch is the rollout's step k0 + k; it reads the actions
// [T][N][adim] at row k0 + k (expert = 1: planned in the kernel, as above) and, after step_finish, writes
// the env's outputs to slice k0 + k of the arrays of R: states and records are bit-identical to a loop of
// mmx_step calls.  No per-phase profile here.
MMX_STEP_KERNEL MMX_STEP_SYM(mmx_env_traj_kernel)(MMXState S, MMXTraj R, const float* actions, int adim, int expert, int base,
                                                  int nsteps, int k0, const int* order) {
  MMX_STEP_KERNEL_ENTRY
  MMX_ENV_WAVE_STEPS(nsteps, NOFSMP,
                     const size_t step = (size_t)(k0 + k);
                     step_begin(S, i, expert ? actions : actions + step * (size_t)S.N * (size_t)adim, adim, expert),
                     traj_record(S, R, i, step * (size_t)S.N + (size_t)i))
}

// The policy's action for the env step that follows (mmx_env_policy_kernel), on the env's wave, out of line like
// the substep.  The observation comes from S.obs[i] in HBM, not from the LDS copy: at the launch's first step
// that copy does not exist, and after an autoreset S.obs holds the new episode's first observation, which is
// what a loop of obs -> policy -> step() feeds the policy.  Before step_begin the whole scratch region is
// free: the normalised input sits at its start, then the two activation buffers.  Lane 0 adds the noise, clamps
// and writes the action row itself; step_begin's lane 0 then reads its own stores back (traj_record's
// argument for the reward), so the row is never handed across lanes through global memory.  No workgroup
// barrier: the helper wave (192 rows) waits at the record-load barrier meanwhile.
#define POL_X 0
#define POL_B0 ((POLICY_NOBS + 3) & ~3)
#define POL_B1 (POL_B0 + POLICY_MAX_WIDTH)
static_assert(POL_B1 + POLICY_MAX_WIDTH <= SCR_FLOATS && POLICY_NOBS == MMX_NOBS, "the policy's scratch exceeds the scratch region");
// The text is stated once, as a macro that defines one out-of-line function per kernel that calls it: policy_act
// for mmx_env_policy_kernel, dagger_policy_act for mmx_env_dagger_kernel.  With ONE caller the optimiser knows where
// the by-reference arguments live (the kernel's own copy of its kernel arguments) and compiles the function for it:
// a second caller of policy_act itself changed its listing and mmx_env_policy_kernel's (tools/isa_same.py: 870 ->
// 866 and 1125 -> 1121 instructions), and the text as a force-inlined function called from two out-of-line wrappers
// kept the counts and changed policy_act's register allocation (as MMX_HELPER_WAVE_STEPS found); these tokens
// pasted into each function leave both listings what the one written-out function gave.  Do not convert it.
#define MMX_DEFINE_POLICY_ACT(name)                                                                                              \
  __device__ __attribute__((noinline)) void name(const MMXState& S, const MmxPolicy& P, const MMXPolicyRec& PR, int i,           \
                                                 unsigned step) {                                                                \
    float* scr = scr_of(g_E);                                                                                                    \
    const float* data = policy_data(P);                                                                                          \
    const float* obs = S.obs + (size_t)i * MMX_NOBS;                                                                             \
    const int shift_off = policy_u(P.shift_off), scale_off = policy_u(P.scale_off);                                              \
    for (int k = LANE; k < MMX_NOBS; k += WG) scr[POL_X + k] = policy_normalise(obs[k], data[shift_off + k], data[scale_off + k]); \
    SYNC();                                                                                                                      \
    const float* mean = policy_forward_wave(P, data, scr + POL_X, scr + POL_B0, scr + POL_B1, LANE);                             \
    if (LANE == 0) {                                                                                                             \
      const int A = P.A;                                                                                                         \
      const size_t row = ((size_t)step * (size_t)S.N + (size_t)i) * (size_t)A;                                                   \
      const float *std = data + P.std_off, *low = data + P.low_off, *high = data + P.high_off;                                   \
      for (int a = 0; a < A; a++) {                                                                                              \
        const float m = mean[a];                                                                                                 \
        float z = 0.f, act = mppi_clamp(m, low[a], high[a]);                                                                     \
        if (P.stochastic) {                                                                                                      \
          z = mppi_draw(P.seed_lo, P.seed_hi, P.call_lo, P.call_hi, step, (uint32_t)i, (uint32_t)a);                             \
          act = policy_action(m, std[a], z, low[a], high[a]);                                                                    \
        }                                                                                                                        \
        PR.actions[row + a] = act;                                                                                               \
        if (PR.mean) PR.mean[row + a] = m;                                                                                       \
        if (PR.noise) PR.noise[row + a] = z;                                                                                     \
      }                                                                                                                          \
    }                                                                                                                            \
  }
MMX_DEFINE_POLICY_ACT(policy_act)
MMX_DEFINE_POLICY_ACT(dagger_policy_act)

// mmx_env_traj_kernel's step loop with the action of every step computed by an MLP policy from the env's own
// observation, inside the launch (mmx_rollout_policy): step k of the launch is the rollout's step k0 + k; before
// step_begin the env's wave evaluates the policy (policy_act) and writes the action row [k0 + k][i] of
// PR.actions, which step_begin then reads as the trajectory kernel reads a given row.  Everything else is that
// kernel's body, so states and records are bit for bit what mmx_rollout_actions gives on the recorded actions.
MMX_STEP_KERNEL MMX_STEP_SYM(mmx_env_policy_kernel)(MMXState S, MMXTraj R, MmxPolicy P, MMXPolicyRec PR, int base, int nsteps,
                                                    int k0, const int* order) {
  MMX_STEP_KERNEL_ENTRY
  MMX_ENV_WAVE_STEPS(nsteps, NOFSMP,
                     const size_t step = (size_t)(k0 + k);
                     policy_act(S, P, PR, i, (unsigned)step);
                     step_begin(S, i, PR.actions + step * (size_t)S.N * (size_t)P.A, P.A, 0),
                     traj_record(S, R, i, step * (size_t)S.N + (size_t)i))
}

// step_begin for a DAgger step (mmx_env_dagger_kernel), out of line and without register saves like it: the
// record load, then on lane 0 the expert's plan, the gate and the decode of the executed action, and step_begin's
// closing SYNC() -- no workgroup barrier, so the helper wave (192 rows) mirrors nothing new.  The FSM expert plans
// at EVERY step, whoever acts: its state only moves when it plans, so it shadows the learner exactly as
// mmx_expert_plan(16) ahead of every mmx_step would, and the label is what that call returns at this state.
// The learner's row is the one policy_act's lane 0 just wrote to D.policy_action (its own stores, read back; it
// may be D.actions itself, so it is read before the executed action is written).  obs_in is the sim's observation
// buffer as policy_act read it: nothing writes S.obs before step_finish.
__device__ __attribute__((noinline)) void dagger_begin(const MMXState& S, const MmxPolicy& P, const MMXDagger& D, int i,
                                                       unsigned step) {
  EnvSh& E = g_E;
  float* act = scr_of(E) + SCR_ACT;  // lane 0's executed action (E.J is free before the substeps)
  const size_t row = (size_t)step * (size_t)S.N + (size_t)i;
  if (D.obs_in)
    for (int k = LANE; k < MMX_NOBS; k += WG) D.obs_in[row * MMX_NOBS + k] = S.obs[(size_t)i * MMX_NOBS + k];
  load_env(S, i, E);
  if (LANE == 0) {
    float lab[4], pol[4];
    expert_plan(S, i, obj_pos(E, EPI(EPI_OBJ)), hand_pos(E), MMX_NSUBSTEP, lab);
    for (int k = 0; k < 4; k++) pol[k] = D.policy_action[row * 4 + k];
    const float u = dagger_uniform(P.seed_lo, P.seed_hi, P.call_lo, P.call_hi, step, (uint32_t)i);
    const int gate = dagger_gate(u, D.beta, pol, lab, D.takeover_dist);
    dagger_select(gate, pol, lab, act);
    for (int k = 0; k < 4; k++) {
      D.actions[row * 4 + k] = act[k];
      if (D.expert_action) D.expert_action[row * 4 + k] = lab[k];
    }
    if (D.gate) D.gate[row] = gate;
    decode_lane0(S, i, E, act);
  }
  SYNC();
}

// mmx_env_policy_kernel's step loop with the FSM expert beside the learner (mmx_rollout_dagger): step k of the
// launch is the rollout's step k0 + k; the env's wave evaluates the policy (policy_act's text, as it stands: the
// learner's action row [k0 + k][i] of PR.actions = D.policy_action), then dagger_begin plans with the expert, records the
// label, draws the gate and steps the env with the expert's action where the gate fires and the learner's where it
// does not.  Everything else is that kernel's body, so states and records are bit for bit what the loop
// mmx_expert_plan(16) -> mmx_step(D.actions[t]) gives.
MMX_STEP_KERNEL MMX_STEP_SYM(mmx_env_dagger_kernel)(MMXState S, MMXTraj R, MmxPolicy P, MMXPolicyRec PR, MMXDagger D, int base,
                                                    int nsteps, int k0, const int* order) {
  MMX_STEP_KERNEL_ENTRY
  MMX_ENV_WAVE_STEPS(nsteps, NOFSMP,
                     const size_t step = (size_t)(k0 + k);
                     dagger_policy_act(S, P, PR, i, (unsigned)step);
                     dagger_begin(S, P, D, i, (unsigned)step),
                     traj_record(S, R, i, step * (size_t)S.N + (size_t)i))
}

// One IK + mj_step substep per launch (mmx_launch_physics, the physics-level harness of mmx_physics_step;
// with SS_GYM the env step's first / last), in the build's own layout like the step kernels above.  With
// the helper wave (192 rows), threads 64..127 run one substep of the fused kernels' helper loop, the sequence
// MMX_HELPER_WAVE_STEPS (above) states: the barrier after the record load, then mj_step_wave's C, K, A, P, Q
// in that order.  Written out here because it differs: one substep, no delay hooks, and the IK only with
// SS_IK; its two barriers C and K are crossed either way, and no path of either wave skips one.
extern "C" __global__ void __launch_bounds__(MMX_STEP_THREADS) MMX_STEP_SYM(mmx_substep_kernel)(MMXState S, const float* action,
                                                                                            int adim, int mode) {
  EnvSh& E = g_E;
  const int i = blockIdx.x;
  if (i >= S.N) return;
#if MMX_STEP_HELPER
  if (threadIdx.x >= 64) {  // the helper wave: the same workgroup barriers as the env's wave below
    XSYNC();                // the record load
    __syncthreads();        // C
    if (mode & SS_IK) ik_wave(E);
    __syncthreads();  // K: the IK has read the kinematics cache; the env wave may overwrite it
    __syncthreads();  // A
    dynamics_wave(E);
    __syncthreads();  // P
    collide_pairs(E, false, 2);
    __syncthreads();  // Q
    return;
  }
#endif
  load_env(S, i, E);
  if ((mode & SS_FIRST) && (mode & SS_GYM) && LANE == 0) take_action_lane0(S, i, E, action, adim, mode & SS_EXPERT);
  SYNC();
#if MMX_STEP_HELPER
  XSYNC();  // the record and the decoded target are in LDS (the helper's IK and dynamics read them)
#endif
  {
    float* stats = E.stats;
    CLK_DECL;
#if !MMX_STEP_HELPER  // (the helper wave's, beside the kinematics: mj_step_wave)
    if (mode & SS_IK) ik_wave(E);  // IK on the kinematics of the previous position stage
    SYNC();
#endif
    CLK(stats, STAT_T_IK);
  }
  mj_step_wave(S.solver_max_iter, S.solver_tol, E, (mode & SS_LAST) ? contacts_dst(S, i) : nullptr);
  if ((mode & SS_LAST) && (mode & SS_GYM)) {
    step_end(S, i, E);
  } else {
    if (LANE == 0) {
      fold_flags(S, i, E);
      if (mode & SS_LAST) {
        EPI(EPI_NCON) = E.ncon;
        EPI(EPI_NEFC) = E.nefc_mj;
      }
    }
  }
  store_env(S, i, E);
}

// ===================================================================== the step kernels' launchers
// Occupancy probe (diagnostics only, never set by the product): MMX_LDS_PAD bytes of dynamic LDS
// per step-kernel workgroup lower the envs per CU (tools/occupancy_probe.sh).
static size_t step_lds_pad() {
  static const size_t pad = [] {
    const char* v = std::getenv("MMX_LDS_PAD");
    return v ? (size_t)std::max(0, std::atoi(v)) : (size_t)0;
  }();
  return pad;
}
// The fused kernels' launch line: one workgroup per env of the launch, `count` of them, on the stream `st`.
template <typename... Params, typename... Args>
static hipError_t launch_fused(void (*kernel)(Params...), int count, hipStream_t st, const Args&... args) {
  hipLaunchKernelGGL(kernel, dim3(count), dim3(MMX_STEP_THREADS), step_lds_pad(), st, args...);
  return hipGetLastError();
}
// envs [base, base+count): independent env ranges may run on separate streams
extern "C" hipError_t MMX_STEP_SYM(mmx_launch_step)(const MMXState* S, const float* action, int adim, int expert, int base,
                                                    int count, int nsteps, hipStream_t st, const int* order) {
  if (count <= 0 || nsteps <= 0) return hipSuccess;
  if (nsteps > 1 && !expert) return hipErrorInvalidValue;  // host actions: one env step per launch
  return launch_fused(MMX_STEP_SYM(mmx_env_step_kernel), count, st, *S, action, adim, expert, base, nsteps, order);
}
#if !MMX_STEP_HELPER
// expert steps of envs [base, base+count) up to the bounds and the budget of B (the one-wave layout only)
extern "C" hipError_t mmx_launch_step_budget(const MMXState* S, const MMXBudget* B, const float* action, int adim, int base,
                                             int count, hipStream_t st, const int* order) {
  if (count <= 0) return hipSuccess;
  if (!B->done || !B->acc || B->round < 0 || B->lo < 0 || B->lo > B->hi) return hipErrorInvalidValue;
  return launch_fused(mmx_env_step_budget_kernel, count, st, *S, *B, action, adim, base, order);
}
#endif
// n substeps of every env, one launch each (mmx_physics_step)
extern "C" hipError_t MMX_STEP_SYM(mmx_launch_physics)(const MMXState* S, int n, int with_ik, hipStream_t st) {
  for (int sub = 0; sub < n; sub++) {
    const int mode = (with_ik ? SS_IK : 0) | (sub == n - 1 ? SS_LAST : 0);
    hipLaunchKernelGGL(MMX_STEP_SYM(mmx_substep_kernel), dim3(S->N), dim3(MMX_STEP_THREADS), 0, st, *S, nullptr, 0, mode);
  }
  return hipGetLastError();
}
// `nsteps` env steps of envs [base, base+count) from the rollout's step k0 on, with per-step actions and record
extern "C" hipError_t MMX_STEP_SYM(mmx_launch_traj)(const MMXState* S, const MMXTraj* R, const float* actions, int adim,
                                                    int expert, int base, int count, int nsteps, int k0, hipStream_t st,
                                                    const int* order) {
  if (count <= 0 || nsteps <= 0) return hipSuccess;
  return launch_fused(MMX_STEP_SYM(mmx_env_traj_kernel), count, st, *S, *R, actions, adim, expert, base, nsteps, k0, order);
}
// `nsteps` env steps of envs [base, base+count) from the rollout's step k0 on, every action from the policy P
extern "C" hipError_t MMX_STEP_SYM(mmx_launch_policy)(const MMXState* S, const MMXTraj* R, const MmxPolicy* P,
                                                      const MMXPolicyRec* PR, int base, int count, int nsteps, int k0,
                                                      hipStream_t st, const int* order) {
  if (count <= 0 || nsteps <= 0) return hipSuccess;
  if (!PR->actions || !P->data) return hipErrorInvalidValue;
  return launch_fused(MMX_STEP_SYM(mmx_env_policy_kernel), count, st, *S, *R, *P, *PR, base, nsteps, k0, order);
}
// `nsteps` DAgger env steps of envs [base, base+count) from the rollout's step k0 on: the policy P acts or the FSM
// expert does, by the gate of D; PR->actions is the learner's row and must be D->policy_action (a four-wide policy)
extern "C" hipError_t MMX_STEP_SYM(mmx_launch_dagger)(const MMXState* S, const MMXTraj* R, const MmxPolicy* P,
                                                      const MMXPolicyRec* PR, const MMXDagger* D, int base, int count,
                                                      int nsteps, int k0, hipStream_t st, const int* order) {
  if (count <= 0 || nsteps <= 0) return hipSuccess;
  if (!D->actions || !D->policy_action || PR->actions != D->policy_action || !P->data || P->A != 4) return hipErrorInvalidValue;
  return launch_fused(MMX_STEP_SYM(mmx_env_dagger_kernel), count, st, *S, *R, *P, *PR, *D, base, nsteps, k0, order);
}
