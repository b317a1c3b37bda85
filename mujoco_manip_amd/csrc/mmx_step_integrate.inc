// Part 6 of mmx_step.inc (an ordered fragment, included there and nowhere else): the end of a substep
// (integrate_wave: implicitfast, then the advance), the IK controller (ik_wave) and mj_step_wave, one whole
// mj_step out of the phases of the parts before it, with the table of the workgroup barriers the env wave and
// the helper wave share.  Relies on the lds part, chol_solve_small / kinematics_wave / dynamics_wave (dynamics),
// the collide_* passes (collision), make_constraints_wave (constraints) and newton_wave and RPL (solver).
// ============================================================================ implicitfast + advance (wave)
// Arm: (M - h qDeriv) qacc = qfrc_smooth + qfrc_constraint with qfrc_constraint = M (x - qacc_s),
// qDeriv = -(damping + actuator kv where the force is unclamped), solved by a register Cholesky
// (rows in lanes 0..8); free bodies take the solver's qacc.  Then semi-implicit Euler and
// free-joint quaternion integration (one lane per cube).
DEV void integrate_wave(EnvSh& E) {
  const int d = min(LANE, 8);
  float arow[9];
  float rhs = E.qfrc[d];
#pragma unroll
  for (int c = 0; c < 9; c++) {
    arow[c] = E.M9[d][c];
    rhs += E.M9[d][c] * (E.x[c] - E.qacc_s[c]);
  }
#pragma unroll
  for (int c = 0; c < 9; c++) {
    float a = arow[c];
    if (c == d) {
      a += kDt * MMX_dof_damping[d];
      if (d < 7 && ((E.act_free >> d) & 1)) a -= kDt * MMX_act_bias[3 * d + 2];
    }
    if (((E.act_free >> 7) & 1) && d >= 7 && c >= 7) {  // tendon actuator kv on the finger pair
      const float bv = MMX_act_bias[3 * 7 + 2];
      a -= kDt * bv * MMX_tendon_coef[d - 7] * MMX_tendon_coef[c - 7];
    }
    arow[c] = a;
  }
  const float qa_arm = chol_solve_small<9>(arow, rhs, 1e-12f);
  bool bad = false;
  if (LANE < 27) {
    const float qa = LANE < 9 ? qa_arm : E.x[LANE];
    // (E.x stays: it is the next solve's warm start, MuJoCo's qacc_warmstart)
    const float v = E.qvel[LANE] + kDt * qa;
    E.qvel[LANE] = v;
    // |v| or |qacc| >= 1e10, Inf or NaN (MuJoCo's mj_checkVel / mj_checkAcc bound mjMAXVAL): an
    // integer test of the bits.  The values pass through an opaque register copy first: the device
    // code is built without NaN / Inf semantics (-ffinite-math-only), under which the compiler may
    // treat a NaN or Inf result of the fp ops above as impossible and fold a test it can see through
    // (ADVICE r04); behind the copy the test reads whatever bits the ALU produced.
    unsigned vb = __float_as_uint(v), qb = __float_as_uint(qa);
    asm volatile("" : "+v"(vb), "+v"(qb));
    bad = (vb & 0x7fffffffu) >= 0x501502F9u || (qb & 0x7fffffffu) >= 0x501502F9u;
    if (LANE < 9) E.qpos[LANE] += kDt * v;
  }
  if (__ballot(bad) != 0ull && LANE == 0) E.flags |= SHF_NAN;
  SYNC();
  if (LANE < 3) {
    const int c = LANE, qa = 9 + 7 * c, da = 9 + 6 * c;
    E.qpos[qa] += kDt * E.qvel[da];
    E.qpos[qa + 1] += kDt * E.qvel[da + 1];
    E.qpos[qa + 2] += kDt * E.qvel[da + 2];
    const V3 w = V3{E.qvel[da + 3], E.qvel[da + 4], E.qvel[da + 5]};
    const float wn = norm(w);
    Q4 q = qnormalize(Q4{E.qpos[qa + 3], E.qpos[qa + 4], E.qpos[qa + 5], E.qpos[qa + 6]});
    if (wn > 0.f) q = qmul(q, qaxisangle(w * (1.f / wn), wn * kDt));
    q = qnormalize(q);
    E.qpos[qa + 3] = q.w; E.qpos[qa + 4] = q.x; E.qpos[qa + 5] = q.y; E.qpos[qa + 6] = q.z;
  }
  SYNC();
}

// ============================================================================ IK (lane 0)
DEV void orientation_error(const M3& Rc, V3& err) {  // controller.py:21-43, atan2 form for fp32
  float Em[9];
  const float T[9] = {0.f, 1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, -1.f};
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Em[3 * r + c] = T[3 * r] * Rc.m[3 * c] + T[3 * r + 1] * Rc.m[3 * c + 1] + T[3 * r + 2] * Rc.m[3 * c + 2];
  const V3 v = V3{Em[7] - Em[5], Em[2] - Em[6], Em[3] - Em[1]};
  const float cs = fminf(fmaxf((Em[0] + Em[4] + Em[8] - 1.f) * 0.5f, -1.f), 1.f);
  const float sn = 0.5f * norm(v);
  const float ang = atan2f(sn, cs);
  if (ang < 1e-6f || sn < 1e-12f) {
    err = V3{0.f, 0.f, 0.f};
    return;
  }
  err = v * (ang / (2.f * sn));
}

DEV void chol6_solve(const float* A, float* x) {
  float L[21];
#pragma unroll
  for (int k = 0; k < 21; k++) L[k] = A[k];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    float s = L[LT(j, j)];
#pragma unroll
    for (int k = 0; k < j; k++) s -= L[LT(j, k)] * L[LT(j, k)];
    const float d = sqrtf(fmaxf(s, 1e-20f)), inv = 1.f / d;
    L[LT(j, j)] = d;
#pragma unroll
    for (int r = j + 1; r < 6; r++) {
      float t = L[LT(r, j)];
#pragma unroll
      for (int k = 0; k < j; k++) t -= L[LT(r, k)] * L[LT(j, k)];
      L[LT(r, j)] = t * inv;
    }
  }
#pragma unroll
  for (int r = 0; r < 6; r++) {
    float s = x[r];
#pragma unroll
    for (int k = 0; k < r; k++) s -= L[LT(r, k)] * x[k];
    x[r] = s / L[LT(r, r)];
  }
#pragma unroll
  for (int r = 5; r >= 0; r--) {
    float s = x[r];
#pragma unroll
    for (int k = r + 1; k < 6; k++) s -= L[LT(k, r)] * x[k];
    x[r] = s / L[LT(r, r)];
  }
}

// DLS IK with nullspace bias on the stale kinematics cache -> ctrl[0:7]
DEV void ik_lane0(EnvSh& E) {
  const V3 tgt = V3{E.target[0], E.target[1], E.target[2]};
  const V3 ee = V3{kin_get(E, KIN_HAND_POS), kin_get(E, KIN_HAND_POS + 1), kin_get(E, KIN_HAND_POS + 2)};
  M3 Rc;
#pragma unroll
  for (int k = 0; k < 9; k++) Rc.m[k] = kin_get(E, KIN_HAND_MAT + k);
  float J[6][7];
#pragma unroll
  for (int d = 0; d < 7; d++) {
    const V3 ax = V3{kin_get(E, KIN_AXIS + 3 * d), kin_get(E, KIN_AXIS + 3 * d + 1), kin_get(E, KIN_AXIS + 3 * d + 2)};
    const V3 an = V3{kin_get(E, KIN_ANCHOR + 3 * d), kin_get(E, KIN_ANCHOR + 3 * d + 1), kin_get(E, KIN_ANCHOR + 3 * d + 2)};
    const V3 jp = cross(ax, ee - an);
    J[0][d] = jp.x; J[1][d] = jp.y; J[2][d] = jp.z;
    J[3][d] = ax.x; J[4][d] = ax.y; J[5][d] = ax.z;
  }
  V3 ori;
  orientation_error(Rc, ori);
  const float e6[6] = {tgt.x - ee.x, tgt.y - ee.y, tgt.z - ee.z, ori.x, ori.y, ori.z};
  float A[21];
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = 0; c <= r; c++) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 7; k++) s += J[r][k] * J[c][k];
      A[LT(r, c)] = s + (r == c ? 1e-3f : 0.f);
    }
  float q[7], b[7];
#pragma unroll
  for (int k = 0; k < 7; k++) {
    q[k] = E.qpos[k];
    b[k] = 0.5f * (kHome[k] - q[k]);
  }
  float y[6], z[6];  // dq = J' A^-1 e + (b - J' A^-1 J b)
#pragma unroll
  for (int r = 0; r < 6; r++) {
    y[r] = e6[r];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 7; k++) s += J[r][k] * b[k];
    z[r] = s;
  }
  chol6_solve(A, y);
  chol6_solve(A, z);
  float dq[7], n2 = 0.f;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    float s = b[k];
#pragma unroll
    for (int r = 0; r < 6; r++) s += J[r][k] * (y[r] - z[r]);
    dq[k] = s;
    n2 += s * s;
  }
  const float nrm = sqrtf(n2);
  const float scl = nrm > 5.0f ? 5.0f / nrm : 1.0f;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    float t = q[k] + dq[k] * scl;
    const float lo = MMX_jnt_range[2 * k], hi = MMX_jnt_range[2 * k + 1];
    if (lo < hi) t = fminf(fmaxf(t, lo), hi);
    E.ctrl[k] = t;
  }
}

// Wave form of ik_lane0: J columns one lane per arm joint, the 6 x 6 DLS system one lane per row
// (register Cholesky), dq = b + J' A^{-1} (e - J b) with b the null-space pull toward home
// (= J' A^{-1} e + (I - J' A^{-1} J) b of controller.py:111-124).  Scratch: E.J (free here).
DEV void ik_wave(EnvSh& E) {
  float* W = scr_of(E) + SCR_IKW;  // J [6][8] at 0, b [8] at 48, e [8] at 56, u [8] at 64
  const V3 ee = V3{kin_get(E, KIN_HAND_POS), kin_get(E, KIN_HAND_POS + 1), kin_get(E, KIN_HAND_POS + 2)};
  if (LANE < 7) {
    const int d = LANE;
    const V3 ax = V3{kin_get(E, KIN_AXIS + 3 * d), kin_get(E, KIN_AXIS + 3 * d + 1), kin_get(E, KIN_AXIS + 3 * d + 2)};
    const V3 an = V3{kin_get(E, KIN_ANCHOR + 3 * d), kin_get(E, KIN_ANCHOR + 3 * d + 1), kin_get(E, KIN_ANCHOR + 3 * d + 2)};
    const V3 jp = cross(ax, ee - an);
    W[0 * 8 + d] = jp.x; W[1 * 8 + d] = jp.y; W[2 * 8 + d] = jp.z;
    W[3 * 8 + d] = ax.x; W[4 * 8 + d] = ax.y; W[5 * 8 + d] = ax.z;
    W[48 + d] = 0.5f * (kHome[d] - E.qpos[d]);
  } else if (LANE == 7) {
    M3 Rc;
#pragma unroll
    for (int k = 0; k < 9; k++) Rc.m[k] = kin_get(E, KIN_HAND_MAT + k);
    V3 ori;
    orientation_error(Rc, ori);
    W[56] = E.target[0] - ee.x; W[57] = E.target[1] - ee.y; W[58] = E.target[2] - ee.z;
    W[59] = ori.x; W[60] = ori.y; W[61] = ori.z;
  }
  SYNC();
  const int r = min(LANE, 5);
  float arow[6], rhs = W[56 + r];
#pragma unroll
  for (int c = 0; c < 6; c++) arow[c] = r == c ? 1e-3f : 0.f;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    const float jr = W[8 * r + k];
#pragma unroll
    for (int c = 0; c < 6; c++) arow[c] = fmaf(jr, W[8 * c + k], arow[c]);
    rhs = fmaf(-jr, W[48 + k], rhs);
  }
  const float u = chol_solve_small<6>(arow, rhs, 1e-20f);
  if (LANE < 6) W[64 + LANE] = u;
  SYNC();
  float dq = 0.f;
  if (LANE < 7) {
    dq = W[48 + LANE];
#pragma unroll
    for (int rr = 0; rr < 6; rr++) dq = fmaf(W[8 * rr + LANE], W[64 + rr], dq);
  }
  const float nrm = sqrtf(wave_sum(dq * dq));
  const float scl = nrm > 5.0f ? 5.0f / nrm : 1.0f;
  if (LANE < 7) {
    float t = E.qpos[LANE] + dq * scl;
    const float lo = MMX_jnt_range[2 * LANE], hi = MMX_jnt_range[2 * LANE + 1];
    if (lo < hi) t = fminf(fmaxf(t, lo), hi);
    E.ctrl[LANE] = t;
  }
  SYNC();
}

// ============================================================================ one mj_step
DEV void mj_step_wave(int max_iter, float tol, EnvSh& E, float* con_dst) {
  float* stats = E.stats;
  CLK_DECL;
#if MMX_STEP_HELPER
  // the env wave and the helper wave (the kernels' helper loop, MMX_HELPER_WAVE_STEPS in mmx_step_kernels.inc,
  // mirrors these workgroup barriers: C, K, A, P, Q in every substep, no path of either wave skips one, and
  // mmx_substep_kernel's helper follows the same sequence).  Between two barriers the waves share
  // LDS read-only, or write disjoint parts of it:
  //   C..K  env: the chain scan in its scratch        helper: the IK (reads the kinematics cache = the
  //                                                   previous position stage's poses; writes ctrl)
  //   K..A  env: writes the poses and S (the cache)   helper: nothing
  //   A..P  env: the prune (reads poses, S, qvel;     helper: the dynamics (reads the same; writes M9,
  //         its displacement bound is its own)        qfrc, qacc_s and its scratch)
  //   P..Q  env: plane and box-box pairs              helper: the GJK / EPA pairs, and with them the axis
  //                                                   cache (mmx_gjk_cache.h; HBM, not LDS): loaded after P,
  //                                                   stored before Q, entry s by the helper's lane s alone
  // The env wave never touches the axis cache: its GJK pairs are those of the step end's robot-obstacle pass
  // (collide_wave(E, true), after the last substep's Q), which runs without it, so no barrier has to order it.
  // (tests/test_helper_layout.py holds either wave back after C and A and compares the results)
  __syncthreads();  // C: the previous substep's state is in LDS; the helper runs the IK
  DELAY_ENV();
  kinematics_wave(E, true);  // (barrier K inside, before the poses are written)
  CLK(stats, STAT_T_KIN);
  __syncthreads();  // A: the kinematics; the helper runs the dynamics beside the broadphase
  DELAY_ENV();
  collide_prune(E, false);
  __syncthreads();  // P: the class lists (and the dynamics); the helper takes the GJK / EPA pairs
  collide_pairs(E, false, 1);
  __syncthreads();  // Q: the helper's contacts (the rank sort orders them by key)
  collide_sort(E);
#else
  kinematics_wave(E);
  CLK(stats, STAT_T_KIN);
  dynamics_wave(E);
  CLK(stats, STAT_T_DYN);
  collide_wave(E, false);
#endif
  CLK(stats, STAT_T_COL);
  if (con_dst) store_contacts(con_dst, E);  // before the row build reuses contact fields
  float mu[RPL];  // the lane's rows' mu (LANE + 64 q), from the row build to the solver
  make_constraints_wave(E, mu);
  CLK(stats, STAT_T_CON);
  float resid = 0.f;
  int exit = 0;
  const int it = newton_wave(E, max_iter, tol, resid, exit, mu);
  CLK(stats, STAT_T_SOLVE);
  integrate_wave(E);
  CLK(stats, STAT_T_INT);
  if (LANE == 0) {
    stats[STAT_NEFC] += (float)E.nefc_mj;  // MuJoCo's rows (pyramid edges), not the stored basis rows
    stats[STAT_NCON] += (float)E.ncon;
    stats[STAT_SOLVER_ITER] += (float)it;
    stats[STAT_SUBSTEPS] += 1.f;
    stats[STAT_RESID] = fmaxf(stats[STAT_RESID], resid);
    // solver exits above tolerance, by cause (no progress in fp32 / iteration cap)
    stats[STAT_EXIT_STALL] += exit == 1 ? 1.f : 0.f;
    stats[STAT_EXIT_CAP] += exit == 2 ? 1.f : 0.f;
#ifdef MMX_PHASE_CLOCK
    if (MMX_PROBE == 12) {  // row / contact count distribution (sizes the LDS row capacity)
      stats[STAT_T_AUX0] = fmaxf(stats[STAT_T_AUX0], (float)E.nefc);  // stored (basis) rows
      stats[STAT_T_AUX1] = fmaxf(stats[STAT_T_AUX1], (float)E.ncon);
      stats[STAT_T_AUX2] += E.nefc > MMX_LDSEFC ? 1.f : 0.f;
      stats[STAT_T_AUX3] += E.nefc > 160 ? 1.f : 0.f;
    }
#endif
  }
  SYNC();
}
