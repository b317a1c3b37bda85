// Part 2 of mmx_step.inc (an ordered fragment, included there and nowhere else): the position and velocity
// stages.  kinematics_lane0 / kinematics_wave (body poses, motion subspaces, the IK's kinematics cache; on
// the 192-row layout the env wave crosses barrier K inside it) and dynamics_wave (RNE bias, composite inertias,
// CRBA, actuator forces, the unconstrained acceleration), with the 16-lane row broadcasts and the small register
// Cholesky (row_bcast, chol_solve_small) that later parts use too.  Relies on the lds part: EnvSh, the scratch
// map, the body-pose accessors and the wave primitives.
// ============================================================================ kinematics (lane 0)
// mj_kinematics + arm motion subspaces (world-origin Plucker).  All joint anchors of this model
// sit at the body origin (jnt_pos = 0).  Also refreshes the IK's kinematics cache (SURVEY A.5).
DEV void kinematics_lane0(EnvSh& E) {
  V3 px[12];
  Q4 pq[12];
  px[0] = V3{0.f, 0.f, 0.f};
  pq[0] = Q4{1.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 1; b <= 11; b++) {
    const int p = MMX_body_parent[b];
    const M3 Rp = qmat(pq[p]);
    V3 pos = px[p] + mul(Rp, V3{MMX_body_pos[3 * b], MMX_body_pos[3 * b + 1], MMX_body_pos[3 * b + 2]});
    Q4 q = qmul(pq[p], Q4{MMX_body_quat[4 * b], MMX_body_quat[4 * b + 1], MMX_body_quat[4 * b + 2], MMX_body_quat[4 * b + 3]});
    const int j = MMX_body_jnt[b];
    if (j >= 0) {
      const V3 axl = V3{MMX_jnt_axis[3 * j], MMX_jnt_axis[3 * j + 1], MMX_jnt_axis[3 * j + 2]};
      const V3 axw = mul(qmat(qnormalize(q)), axl);
      const float qv = E.qpos[j];
      if (MMX_jnt_type[j] == 3) {  // hinge
        q = qmul(q, qaxisangle(axl, qv));
        const V3 lin = cross(pos, axw);
        E.S[j][0] = axw.x; E.S[j][1] = axw.y; E.S[j][2] = axw.z;
        E.S[j][3] = lin.x; E.S[j][4] = lin.y; E.S[j][5] = lin.z;
      } else {  // slide
        E.S[j][0] = 0.f; E.S[j][1] = 0.f; E.S[j][2] = 0.f;
        E.S[j][3] = axw.x; E.S[j][4] = axw.y; E.S[j][5] = axw.z;
        pos = pos + axw * qv;
      }
    }
    q = qnormalize(q);
    px[b] = pos;
    pq[b] = q;
    const M3 R = qmat(q);
    const int s = b - 1;
    E.bx[s][0] = pos.x; E.bx[s][1] = pos.y; E.bx[s][2] = pos.z;
#pragma unroll
    for (int k = 0; k < 9; k++) E.bR[s][k] = R.m[k];
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const int qa = 9 + 7 * c;
    const M3 R = qmat(qnormalize(Q4{E.qpos[qa + 3], E.qpos[qa + 4], E.qpos[qa + 5], E.qpos[qa + 6]}));
    const int s = 11 + c;
    E.bx[s][0] = E.qpos[qa]; E.bx[s][1] = E.qpos[qa + 1]; E.bx[s][2] = E.qpos[qa + 2];
#pragma unroll
    for (int k = 0; k < 9; k++) E.bR[s][k] = R.m[k];
  }
}

// Wave form of kinematics_lane0: one lane per body.  Each arm body first builds its local
// transform (static offset x joint), then the chain is composed by pointer jumping (4 rounds
// cover the 10-deep finger chain): T_b <- T_anc(b) o T_b, anc(b) <- anc(anc(b)).  Cubes read their
// free joints directly.  Results equal kinematics_lane0 up to fp32 association order.
// in_step (mj_step_wave of the two-wave layout only): workgroup barrier K before the write-out.  The
// poses written there ARE the IK's kinematics cache (kin_ref), which the helper wave's IK of this substep
// reads as the previous position stage left it; the helper crosses K once its IK is done.
DEV void kinematics_wave(EnvSh& E, bool in_step = false) {
  float* T = scr_of(E);  // [12][8] scan scratch: q (4), p (3), ancestor
  const int b = LANE + 1;    // lanes 0..10 -> arm bodies 1..11
  Q4 q = Q4{1.f, 0.f, 0.f, 0.f};
  V3 p = V3{0.f, 0.f, 0.f};
  int anc = 0;
  if (LANE < 11) {
    p = V3{MMX_body_pos[3 * b], MMX_body_pos[3 * b + 1], MMX_body_pos[3 * b + 2]};
    q = Q4{MMX_body_quat[4 * b], MMX_body_quat[4 * b + 1], MMX_body_quat[4 * b + 2], MMX_body_quat[4 * b + 3]};
    const int j = MMX_body_jnt[b];
    if (j >= 0) {
      const V3 axl = V3{MMX_jnt_axis[3 * j], MMX_jnt_axis[3 * j + 1], MMX_jnt_axis[3 * j + 2]};
      const float qv = E.qpos[j];
      if (MMX_jnt_type[j] == 3) q = qmul(q, qaxisangle(axl, qv));  // hinge
      else p = p + mul(qmat(qnormalize(q)), axl) * qv;             // slide along the joint axis
    }
    anc = MMX_body_parent[b];
  }
#pragma unroll
  for (int round = 0; round < 4; round++) {
    if (LANE < 11) {
      float* t = T + 8 * b;
      t[0] = q.w; t[1] = q.x; t[2] = q.y; t[3] = q.z;
      t[4] = p.x; t[5] = p.y; t[6] = p.z;
      t[7] = __int_as_float(anc);
    }
    SYNC();
    if (LANE < 11 && anc != 0) {
      const float* t = T + 8 * anc;
      const Q4 qa = Q4{t[0], t[1], t[2], t[3]};
      const V3 pa = V3{t[4], t[5], t[6]};
      const int aa = __float_as_int(t[7]);
      p = pa + mul(qmat(qa), p);
      q = qnormalize(qmul(qa, q));
      anc = aa;
    }
    SYNC();
  }
#if MMX_STEP_HELPER
  if (in_step) __syncthreads();  // K: the helper's IK has read the cache (uniform: every lane of the env wave)
#endif
  if (LANE < 11) {
    q = qnormalize(q);
    const M3 R = qmat(q);
    const int s = b - 1;
    E.bx[s][0] = p.x; E.bx[s][1] = p.y; E.bx[s][2] = p.z;
#pragma unroll
    for (int k = 0; k < 9; k++) E.bR[s][k] = R.m[k];
    const int j = MMX_body_jnt[b];
    if (j >= 0) {
      const V3 axw = mul(R, V3{MMX_jnt_axis[3 * j], MMX_jnt_axis[3 * j + 1], MMX_jnt_axis[3 * j + 2]});
      if (MMX_jnt_type[j] == 3) {
        const V3 lin = cross(p, axw);
        E.S[j][0] = axw.x; E.S[j][1] = axw.y; E.S[j][2] = axw.z;
        E.S[j][3] = lin.x; E.S[j][4] = lin.y; E.S[j][5] = lin.z;
      } else {
        E.S[j][0] = 0.f; E.S[j][1] = 0.f; E.S[j][2] = 0.f;
        E.S[j][3] = axw.x; E.S[j][4] = axw.y; E.S[j][5] = axw.z;
      }
    }
  } else if (LANE < 14) {  // cubes: free joints
    const int c = LANE - 11, qa = 9 + 7 * c;
    const M3 R = qmat(qnormalize(Q4{E.qpos[qa + 3], E.qpos[qa + 4], E.qpos[qa + 5], E.qpos[qa + 6]}));
    const int s = 11 + c;
    E.bx[s][0] = E.qpos[qa]; E.bx[s][1] = E.qpos[qa + 1]; E.bx[s][2] = E.qpos[qa + 2];
#pragma unroll
    for (int k = 0; k < 9; k++) E.bR[s][k] = R.m[k];
  }
  SYNC();
}

// ============================================================================ dynamics
DEV RI body_inertia(const EnvSh& E, int b) {
  const V3 x = body_x(E, b);
  const M3 R = body_R(E, b);
  const float m = MMX_body_mass[b];
  const V3 c = x + mul(R, V3{MMX_body_ipos[3 * b], MMX_body_ipos[3 * b + 1], MMX_body_ipos[3 * b + 2]});
  M3 Ib;
#pragma unroll
  for (int k = 0; k < 9; k++) Ib.m[k] = MMX_body_inertia[9 * b + k];
  const M3 T = mul(R, Ib);
  float Ic[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int cc = 0; cc < 3; cc++) Ic[3 * r + cc] = T.m[3 * r] * R.m[3 * cc] + T.m[3 * r + 1] * R.m[3 * cc + 1] + T.m[3 * r + 2] * R.m[3 * cc + 2];
  RI I;
  I.m = m;
  I.h = c * m;
  const float cc2 = dot(c, c);
  I.J[0] = Ic[0] + m * (cc2 - c.x * c.x);
  I.J[1] = Ic[4] + m * (cc2 - c.y * c.y);
  I.J[2] = Ic[8] + m * (cc2 - c.z * c.z);
  I.J[3] = Ic[1] - m * c.x * c.y;
  I.J[4] = Ic[2] - m * c.x * c.z;
  I.J[5] = Ic[5] - m * c.y * c.z;
  return I;
}
DEV void ri_store(float* d, const RI& I) {
  d[0] = I.m; d[1] = I.h.x; d[2] = I.h.y; d[3] = I.h.z;
#pragma unroll
  for (int k = 0; k < 6; k++) d[4 + k] = I.J[k];
}
DEV RI ri_load(const float* d) {
  RI I;
  I.m = d[0];
  I.h = V3{d[1], d[2], d[3]};
#pragma unroll
  for (int k = 0; k < 6; k++) I.J[k] = d[4 + k];
  return I;
}

#define LT(r, c) ((r) * ((r) + 1) / 2 + (c))

// RNE bias of the arm + composite inertias (for CRBA), one lane per moving arm body (2..11).  A
// body's velocity and acceleration are running sums over the joints on its root path (arm_anc),
// its force is local.  Lane l < 10 holds body b = 11 - l (the fingers 11, 10, then the chain 9..2),
// so a body's subtree (bodies >= b for b <= 9, itself for a finger) is an inclusive prefix over
// lanes 0..l: the backward pass and the composite inertias are 16 DPP row_shr scans in registers.
// Scratch at SCR_DYN: subtree force (6) per body at 16 * 12, composite inertias at SCR_IC.
DEV float shr_add_scan(float v) {  // inclusive prefix sum over the lanes of each 16-lane row
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xF, 0xF, false));  // row_shr:1
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xF, 0xF, false));  // row_shr:2
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xF, 0xF, false));  // row_shr:4
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xF, 0xF, false));  // row_shr:8
  return v;
}
// An arm body's velocity and the speed that enters the broadphase list's displacement bound
// (list_disp_next), in fmaf with reassociation and contraction off: the 128-row build takes the bound
// from the RNE's velocities, the two-wave build's env wave computes them itself beside the helper's RNE
// (arm_body_speed), and the two are separate compiles under -fassociative-math whose bounds, and so
// their list-use decisions, must agree to the bit.
DEV SV sv_fma_exact(SV s, float q, SV a) {  // a + s q
#pragma clang fp reassociate(off) contract(off)
  return SV{V3{fmaf(s.w.x, q, a.w.x), fmaf(s.w.y, q, a.w.y), fmaf(s.w.z, q, a.w.z)},
            V3{fmaf(s.v.x, q, a.v.x), fmaf(s.v.y, q, a.v.y), fmaf(s.v.z, q, a.v.z)}};
}
// |velocity of the body origin p| + |angular velocity| x crad (vel: world-origin Plucker, v + w x p)
DEV float body_speed_exact(SV vel, V3 p, float crad) {
#pragma clang fp reassociate(off) contract(off)
  const float ox = fmaf(vel.w.y, p.z, fmaf(-vel.w.z, p.y, vel.v.x));
  const float oy = fmaf(vel.w.z, p.x, fmaf(-vel.w.x, p.z, vel.v.y));
  const float oz = fmaf(vel.w.x, p.y, fmaf(-vel.w.y, p.x, vel.v.z));
  return fmaf(sqrtf(fmaf(vel.w.x, vel.w.x, fmaf(vel.w.y, vel.w.y, vel.w.z * vel.w.z))), crad,
              sqrtf(fmaf(ox, ox, fmaf(oy, oy, oz * oz))));
}
#if MMX_STEP_HELPER
// the env wave's own copy of the RNE's velocity sums (lanes 0..9: the moving arm bodies 11..2)
DEV float arm_body_speed(const EnvSh& E) {
  float s = 0.f;
  if (LANE < 10) {
    const int b = 11 - LANE;
    SV vel = SV{V3{0.f, 0.f, 0.f}, V3{0.f, 0.f, 0.f}};
#pragma unroll
    for (int d = 0; d < 9; d++)
      if (arm_anc(d, b)) vel = sv_fma_exact(load_S(E, d), E.qvel[d], vel);
    s = body_speed_exact(vel, body_x(E, b), E.crad);
  }
  return s;
}
#endif
DEV void rne_wave(EnvSh& E) {
  float* F = scr_of(E) + SCR_DYN;
  const int b = 11 - LANE;
  float fi[16];  // the body's force (6), then its inertia (m, h, J: 10)
#pragma unroll
  for (int m = 0; m < 16; m++) fi[m] = 0.f;
#if !MMX_STEP_HELPER
  float spd = 0.f;  // for collide_prune's displacement bound
#endif
  if (LANE < 10) {
    const RI Ib = body_inertia(E, b);
    SV vel = SV{V3{0.f, 0.f, 0.f}, V3{0.f, 0.f, 0.f}};
    SV acc = SV{V3{0.f, 0.f, 0.f}, V3{0.f, 0.f, -MMX_GRAVITY_Z}};  // base acceleration = -gravity
#pragma unroll
    for (int d = 0; d < 9; d++) {
      if (arm_anc(d, b)) {
        const SV Sd = load_S(E, d);
        const float qd = E.qvel[d];
        acc = acc + cross_motion(vel, Sd * qd);
        vel = sv_fma_exact(Sd, qd, vel);
      }
    }
#if !MMX_STEP_HELPER
    spd = body_speed_exact(vel, body_x(E, b), E.crad);
#endif
    const SV f = rimul(Ib, acc) + cross_force(vel, rimul(Ib, vel));
    fi[0] = f.w.x; fi[1] = f.w.y; fi[2] = f.w.z; fi[3] = f.v.x; fi[4] = f.v.y; fi[5] = f.v.z;
    ri_store(fi + 6, Ib);
  }
#pragma unroll
  for (int m = 0; m < 16; m++) {  // subtree sums (lanes >= 10 hold zeros and come after)
    const float sm = shr_add_scan(fi[m]);
    fi[m] = LANE == 1 ? fi[m] : sm;  // finger 10: its own subtree only (finger 11 sits before it)
  }
  if (LANE < 10) {
#pragma unroll
    for (int m = 0; m < 10; m++) (scr_of(E) + SCR_IC)[10 * b + m] = fi[6 + m];
    float* o = F + 16 * 12 + 6 * b;
#pragma unroll
    for (int m = 0; m < 6; m++) o[m] = fi[m];
  }
  SYNC();
  if (LANE < 9) {
    const float* o = F + 16 * 12 + 6 * MMX_jnt_body[LANE];
    (scr_of(E) + SCR_BIAS)[LANE] = sdot(load_S(E, LANE), SV{V3{o[0], o[1], o[2]}, V3{o[3], o[4], o[5]}});
  }
#if !MMX_STEP_HELPER
  spd = wave_max(spd);
  if (LANE == 0) E.cspd = spd;
#endif
  SYNC();
}

// DPP row_newbcast:K, the value of lane K of each 16-lane row in every lane of that row
template <int K>
DEV float row_bcast_t(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + K, 0xF, 0xF, true));
}
// k is a constant of a fully unrolled loop at every call: the switch folds to one DPP move
DEV float row_bcast(float v, int k) {
  switch (k) {
    case 0: return row_bcast_t<0>(v);
    case 1: return row_bcast_t<1>(v);
    case 2: return row_bcast_t<2>(v);
    case 3: return row_bcast_t<3>(v);
    case 4: return row_bcast_t<4>(v);
    case 5: return row_bcast_t<5>(v);
    case 6: return row_bcast_t<6>(v);
    case 7: return row_bcast_t<7>(v);
    default: return row_bcast_t<8>(v);
  }
}
// broadcast of lane k's value (k < 16) to the lanes of DPP row 0 that hold the small system: one
// row_newbcast (a VGPR result, no SGPR round trip and its hazard nops; v_readlane measured slower)
DEV float small_bcast(float v, int k) { return row_bcast(v, k); }

// (A^{-1} v)_j in lane j for a small SPD A given by rows (lane j holds row j in arow[0..N), N <= 9:
// the rows sit in DPP row 0; lanes of rows 1..3 compute values nobody reads).  Right-looking
// Cholesky with lane broadcasts; lane k keeps column k of L (selects) for the transposed solve.
// eps: pivot floor.  The arithmetic is the same in either broadcast form (bit-identical results).
template <int N>
DEV float chol_solve_small(const float* arow, float v, float eps) {
  static_assert(N <= 9, "row_bcast covers lanes 0..8");
  const int j = LANE & 15;
  float h[N], c[N], dinv[N];
#pragma unroll
  for (int i = 0; i < N; i++) {
    h[i] = arow[i];
    c[i] = 0.f;
  }
#pragma unroll
  for (int k = 0; k < N; k++) {
    const float d = fmaxf(small_bcast(h[k], k), eps);
    const float inv = __builtin_amdgcn_rsqf(d), sd = d * inv;
    dinv[k] = inv;
    const float l = j == k ? sd : h[k] * inv;
    h[k] = l;
    c[k] = j == k ? sd : c[k];
#pragma unroll
    for (int i = k + 1; i < N; i++) {
      const float li = small_bcast(l, i);
      h[i] = fmaf(-li, l, h[i]);
      c[i] = j == k ? li : c[i];
    }
  }
  float y = j < N ? v : 0.f;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const float yk = small_bcast(y, k) * dinv[k];
    y = j == k ? yk : (j > k ? fmaf(-h[k], yk, y) : y);
  }
#pragma unroll
  for (int k = N - 1; k >= 0; k--) {
    const float zk = small_bcast(y, k) * dinv[k];
    y = j == k ? zk : (j < k ? fmaf(-c[k], zk, y) : y);
  }
  return y;
}

// whole wave: mass matrix (CRBA entries in parallel), smooth forces, qacc_smooth
DEV void dynamics_wave(EnvSh& E) {
  float* stats = E.stats;
  CLK_DECL;
  rne_wave(E);
  PROBE(11, stats, STAT_T_AUX0);
  if (LANE < 45) {
    int d, e;
    tri_index(LANE, d, e);
    float v = 0.f;
    if (e == d || (e <= 6 && !(d == 8 && e == 7))) {  // fingers 7, 8 are siblings
      const RI Ic = ri_load(scr_of(E) + SCR_IC + 10 * MMX_jnt_body[d]);
      v = sdot(load_S(E, e), rimul(Ic, load_S(E, d)));
    }
    if (d == e) v += MMX_dof_armature[d];
    E.M9[d][e] = v;
    E.M9[e][d] = v;
  }  // (the cubes' diagonal blocks are model constants: mass_cube)
  SYNC();
  PROBE(11, stats, STAT_T_AUX1);
  // smooth force: passive damping - bias + actuation (arm; one lane per actuator, then per dof),
  // gravity + gyroscopic (cubes, one lane each); arm qacc_smooth = M_arm^{-1} qfrc by a register
  // Cholesky (rows in lanes 0..8)
  float* af = scr_of(E) + SCR_AF;  // actuator forces
  bool unclamped = false;
  if (LANE < 8) {
    const int a = LANE;
    const float c = fminf(fmaxf(E.ctrl[a], MMX_act_ctrlrange[2 * a]), MMX_act_ctrlrange[2 * a + 1]);
    const int j = MMX_act_trn_joint[a];
    const float tlen = MMX_tendon_coef[0] * E.qpos[7] + MMX_tendon_coef[1] * E.qpos[8];
    const float tvel = MMX_tendon_coef[0] * E.qvel[7] + MMX_tendon_coef[1] * E.qvel[8];
    const float len = j >= 0 ? E.qpos[j] : tlen, vel = j >= 0 ? E.qvel[j] : tvel;
    float f = MMX_act_gain[a] * c + MMX_act_bias[3 * a] + MMX_act_bias[3 * a + 1] * len + MMX_act_bias[3 * a + 2] * vel;
    unclamped = f > MMX_act_forcerange[2 * a] && f < MMX_act_forcerange[2 * a + 1];
    af[a] = fminf(fmaxf(f, MMX_act_forcerange[2 * a]), MMX_act_forcerange[2 * a + 1]);
  }
  const unsigned free_mask = (unsigned)__ballot(unclamped);
  if (LANE == 0) E.act_free = (int)free_mask;
  SYNC();
  float qf = 0.f;
  if (LANE < 9) {
    const int d = LANE;
    qf = -MMX_dof_damping[d] * E.qvel[d] - (scr_of(E) + SCR_BIAS)[d];
#pragma unroll
    for (int a = 0; a < 8; a++) {  // actuator order as the serial accumulation
      const int j = MMX_act_trn_joint[a];
      if (j >= 0) qf += j == d ? af[a] : 0.f;
      else qf += d == 7 ? MMX_tendon_coef[0] * af[a] : (d == 8 ? MMX_tendon_coef[1] * af[a] : 0.f);
    }
    E.qfrc[d] = qf;
  } else if (LANE < 12) {  // free body with com at the origin: gravity + w x (I w)
    const int c = LANE - 9, b = 16 + c, da = 9 + 6 * c;
    const float I0 = MMX_body_inertia[9 * b], I1 = MMX_body_inertia[9 * b + 4], I2 = MMX_body_inertia[9 * b + 8];
    const V3 w = V3{E.qvel[da + 3], E.qvel[da + 4], E.qvel[da + 5]};
    const V3 gyro = cross(w, V3{I0 * w.x, I1 * w.y, I2 * w.z});
    const float m = MMX_body_mass[b];
    E.qfrc[da] = 0.f; E.qfrc[da + 1] = 0.f; E.qfrc[da + 2] = MMX_GRAVITY_Z * m;
    E.qfrc[da + 3] = -gyro.x; E.qfrc[da + 4] = -gyro.y; E.qfrc[da + 5] = -gyro.z;
    E.qacc_s[da] = 0.f; E.qacc_s[da + 1] = 0.f; E.qacc_s[da + 2] = MMX_GRAVITY_Z;
    E.qacc_s[da + 3] = -gyro.x / I0; E.qacc_s[da + 4] = -gyro.y / I1; E.qacc_s[da + 5] = -gyro.z / I2;
  }
  float arow[9];
  const int jr = min(LANE, 8);
#pragma unroll
  for (int e = 0; e < 9; e++) arow[e] = E.M9[jr][e];
  PROBE(11, stats, STAT_T_AUX2);
  const float xs = chol_solve_small<9>(arow, qf, 1e-12f);
  if (LANE < 9) E.qacc_s[LANE] = xs;
  SYNC();
  PROBE(11, stats, STAT_T_AUX3);
}
