// Part 7 of mmx_step.inc (an ordered fragment, included there and nowhere else): everything around the physics.
// numpy's PCG64 stream, bit for bit; the task layer on lane 0 (EPI / EPF, the episode record's fields of env i;
// observation, reset and randomisation, reward, the FSM expert's plan, the action decode); and record I/O
// between the sim's env-major buffers and LDS (load_env / store_env / store_obs).  The kernels that exist once
// (mmx_kernels.hip) use it as the fused kernels do.  Relies on the lds part (EnvSh, obs_of, the kinematics cache)
// and on mmx_state.h for MMXState and the record's indices.
// ============================================================================ RNG (numpy PCG64)
struct Pcg {
  unsigned long long shi, slo, ihi, ilo;
};
DEV unsigned long long pcg_next64(Pcg& r) {
  const unsigned long long MH = 0x2360ED051FC65DA4ull, ML = 0x4385DF649FCCF645ull;
  const unsigned long long lo = r.slo * ML;
  unsigned long long hi = __umul64hi(r.slo, ML) + r.slo * MH + r.shi * ML;
  const unsigned long long nlo = lo + r.ilo;
  hi += r.ihi + (nlo < lo ? 1ull : 0ull);
  r.slo = nlo;
  r.shi = hi;
  const unsigned long long x = hi ^ nlo;
  const unsigned rot = (unsigned)(hi >> 58);
  return (x >> rot) | (x << ((64u - rot) & 63u));
}
DEV double pcg_double(Pcg& r) { return (double)(pcg_next64(r) >> 11) * (1.0 / 9007199254740992.0); }

// Generator.integers(high): buffered 32-bit Lemire on next_uint32 (low half first)
DEV int pcg_integers(Pcg& r, int& has32, unsigned& buf32, int high) {
  const unsigned rng = (unsigned)(high - 1);
  if (rng == 0) return 0;
  auto next32 = [&]() -> unsigned {
    if (has32) {
      has32 = 0;
      return buf32;
    }
    const unsigned long long v = pcg_next64(r);
    has32 = 1;
    buf32 = (unsigned)(v >> 32);
    return (unsigned)v;
  };
  const unsigned excl = rng + 1;
  unsigned long long m = (unsigned long long)next32() * excl;
  unsigned left = (unsigned)m;
  if (left < excl) {
    const unsigned thr = (0xFFFFFFFFu - rng) % excl;
    while (left < thr) {
      m = (unsigned long long)next32() * excl;
      left = (unsigned)m;
    }
  }
  return (int)(m >> 32);
}

// ============================================================================ task layer (lane 0)
#define EPI(f) S.epi[(size_t)i * EPI_N + (f)]
#define EPF(f) S.epf[(size_t)i * EPF_N + (f)]

DEV V3 obj_pos(const EnvSh& E, int o) { return V3{E.qpos[9 + 7 * o], E.qpos[10 + 7 * o], E.qpos[11 + 7 * o]}; }
DEV V3 bin_pos(int bn) {
  const int b = kBinBody[bn];  // static bins: body origin = constant body pos (parent = world)
  return V3{MMX_body_pos[3 * b], MMX_body_pos[3 * b + 1], MMX_body_pos[3 * b + 2]};
}
DEV V3 hand_pos(const EnvSh& E) { return V3{kin_get(E, KIN_HAND_POS), kin_get(E, KIN_HAND_POS + 1), kin_get(E, KIN_HAND_POS + 2)}; }
DEV M3 hand_R(const EnvSh& E) {
  M3 R;
#pragma unroll
  for (int k = 0; k < 9; k++) R.m[k] = kin_get(E, KIN_HAND_MAT + k);
  return R;
}

DEV void project(V3 p, V3 cx, const M3& cR, float fovy_deg, float* out) {  // cameras.py:56-104
  const float t = tanf(fovy_deg * (3.14159265358979f / 180.f) * 0.5f);
  const V3 cc = mulT(cR, p - cx);
  float depth = cc.z;
  if (fabsf(depth) < 1e-6f) depth = 1e-6f;
  // px / S = f x / (depth S) + 1/2 with f = (S/2) / tan(fovy/2): independent of the image size
  out[0] = cc.x / (depth * 2.f * t) + 0.5f;
  out[1] = -cc.y / (depth * 2.f * t) + 0.5f;
}
DEV void camera_pose(int cam, V3 hx, const M3& hR, V3& cx, M3& cR) {
  const M3 lq = qmat(Q4{MMX_cam_quat[4 * cam], MMX_cam_quat[4 * cam + 1], MMX_cam_quat[4 * cam + 2], MMX_cam_quat[4 * cam + 3]});
  const V3 lp = V3{MMX_cam_pos[3 * cam], MMX_cam_pos[3 * cam + 1], MMX_cam_pos[3 * cam + 2]};
  if (MMX_cam_body[cam] == 0) {
    cx = lp;
    cR = lq;
  } else {
    cx = hx + mul(hR, lp);
    cR = mul(hR, lq);
  }
}
DEV void rotmat_to_quat_xyzw(const float* R, float* q) {  // pose_utils.py:48-82 (branch-exact)
  const float tr = R[0] + R[4] + R[8];
  float s, w, x, y, z;
  if (tr > 0.f) {
    s = 2.f * sqrtf(tr + 1.f);
    w = 0.25f * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    s = 2.f * sqrtf(1.f + R[0] - R[4] - R[8]);
    w = (R[7] - R[5]) / s; x = 0.25f * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    s = 2.f * sqrtf(1.f + R[4] - R[0] - R[8]);
    w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25f * s; z = (R[5] + R[7]) / s;
  } else {
    s = 2.f * sqrtf(1.f + R[8] - R[0] - R[4]);
    w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25f * s;
  }
  q[0] = x; q[1] = y; q[2] = z; q[3] = w;
}

// numeric observation (gym_env.py:283-339, 85 floats) into E.obs
DEV void obs_lane0(const MMXState& S, int i, EnvSh& E) {
  const V3 hx = hand_pos(E);
  const M3 hR = hand_R(E);
  float* o = obs_of(E);
  const float g = E.ctrl[7] / 255.f;
  o[0] = hx.x; o[1] = hx.y; o[2] = hx.z; o[3] = g;
#pragma unroll
  for (int k = 0; k < 7; k++) o[4 + k] = E.qpos[k];
  float Ri[9];
#pragma unroll
  for (int k = 0; k < 9; k++) Ri[k] = EPF(EPF_TINIT + k);
  const V3 pi = V3{EPF(EPF_TINIT + 9), EPF(EPF_TINIT + 10), EPF(EPF_TINIT + 11)};
  float Rr[9];  // T_rel = inv(T_init) T_cur
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Rr[3 * r + c] = Ri[r] * hR.m[c] + Ri[3 + r] * hR.m[3 + c] + Ri[6 + r] * hR.m[6 + c];
  const V3 dp = hx - pi;
  const V3 pr = V3{Ri[0] * dp.x + Ri[3] * dp.y + Ri[6] * dp.z, Ri[1] * dp.x + Ri[4] * dp.y + Ri[7] * dp.z,
                   Ri[2] * dp.x + Ri[5] * dp.y + Ri[8] * dp.z};
  for (int rel = 0; rel < 2; rel++) {
    const float* R = rel ? Rr : hR.m;
    const V3 p = rel ? pr : hx;
    float* q8 = o + (rel ? 29 : 11);
    float* r10 = o + (rel ? 37 : 19);
    float q[4];
    rotmat_to_quat_xyzw(R, q);
    q8[0] = p.x; q8[1] = p.y; q8[2] = p.z;
    q8[3] = q[0]; q8[4] = q[1]; q8[5] = q[2]; q8[6] = q[3]; q8[7] = g;
    r10[0] = p.x; r10[1] = p.y; r10[2] = p.z;
#pragma unroll
    for (int k = 0; k < 6; k++) r10[3 + k] = R[k];
    r10[9] = g;
  }
  const int ob = EPI(EPI_OBJ), bn = EPI(EPI_BIN);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    o[47 + k] = (k == bn) ? 1.f : 0.f;
    o[50 + k] = (k == ob) ? 1.f : 0.f;
  }
  const V3 kp[7] = {obj_pos(E, 0), obj_pos(E, 1), obj_pos(E, 2), bin_pos(0), bin_pos(1), bin_pos(2), hx};
  V3 cx;
  M3 cR;
  camera_pose(MMX_CAM_OVERHEAD, hx, hR, cx, cR);
#pragma unroll
  for (int k = 0; k < 7; k++) project(kp[k], cx, cR, MMX_cam_fovy[MMX_CAM_OVERHEAD], o + 53 + 2 * k);
  camera_pose(MMX_CAM_WRIST, hx, hR, cx, cR);
#pragma unroll
  for (int k = 0; k < 7; k++) project(kp[k], cx, cR, MMX_cam_fovy[MMX_CAM_WRIST], o + 67 + 2 * k);
#pragma unroll
  for (int k = 0; k < 4; k++) o[81 + k] = EPF(EPF_TGTKP + k);
}

// reset (gym_env.py:477-534) of the env in E; S.rng may just have been re-seeded by the host
DEV void reset_lane0(const MMXState& S, int i, EnvSh& E, int task_override) {
#pragma unroll
  for (int k = 0; k < 30; k++) E.qpos[k] = MMX_key_qpos[k];
#pragma unroll
  for (int k = 0; k < 27; k++) {
    E.qvel[k] = 0.f;
    E.x[k] = 0.f;
  }
#pragma unroll
  for (int k = 0; k < 8; k++) E.ctrl[k] = MMX_key_ctrl[k];
  Pcg r = Pcg{S.rng[4 * (size_t)i], S.rng[4 * (size_t)i + 1], S.rng[4 * (size_t)i + 2], S.rng[4 * (size_t)i + 3]};
  int has32 = EPI(EPI_RNG_HAS32);
  unsigned buf32 = S.rng32[i];
  bool ok = true;  // the spawn sampling succeeded (or did not run)
  if (S.randomize) {  // randomization.py:70-98 (fp64 draws, numpy-identical stream)
    double xs[3] = {0, 0, 0}, ys[3] = {0, 0, 0};
    ok = false;
    for (int att = 0; att < 1000 && !ok; att++) {
      for (int k = 0; k < 3; k++) xs[k] = (double)S.spawn_x0 + ((double)S.spawn_x1 - (double)S.spawn_x0) * pcg_double(r);
      for (int k = 0; k < 3; k++) ys[k] = (double)S.spawn_y0 + ((double)S.spawn_y1 - (double)S.spawn_y0) * pcg_double(r);
      ok = true;
      for (int a = 0; a < 3; a++)
        for (int b = a + 1; b < 3; b++) {
          const double dx = xs[a] - xs[b], dy = ys[a] - ys[b];
          if (dx * dx + dy * dy < 0.08 * 0.08) ok = false;
        }
    }
    // exhausted (randomization.py:84-87 raises RuntimeError before touching qpos or drawing the task):
    // the cubes stay at the keyframe, the task draw is skipped (the stream stays the reference's), the
    // env's error bit and the sim's fault word are set; mmx_reset / mmx_synchronize turn the fault into
    // MMX_ESAMPLING and the facades into the reference's RuntimeError
    if (!ok) {
      EPI(EPI_ERROR) |= ERR_SAMPLING;
      atomicOr(S.fault, (int)ERR_SAMPLING);
    }
    for (int k = 0; k < 3 && ok; k++) {
      const int qa = 9 + 7 * k;
      E.qpos[qa] = (float)xs[k]; E.qpos[qa + 1] = (float)ys[k]; E.qpos[qa + 2] = 0.26f;
      E.qpos[qa + 3] = 1.f; E.qpos[qa + 4] = 0.f; E.qpos[qa + 5] = 0.f; E.qpos[qa + 6] = 0.f;
    }
  }
  kinematics_lane0(E);
  const V3 hx = hand_pos(E);
#pragma unroll
  for (int k = 0; k < 9; k++) EPF(EPF_TINIT + k) = kin_get(E, KIN_HAND_MAT + k);
  EPF(EPF_TINIT + 9) = hx.x; EPF(EPF_TINIT + 10) = hx.y; EPF(EPF_TINIT + 11) = hx.z;
  EPI(EPI_STEP) = 0;
  EPI(EPI_FLAGS) = 0;
#pragma unroll
  for (int k = 0; k < 5; k++) EPF(EPF_HWM + k) = 0.f;
  EPF(EPF_EP_RETURN) = 0.f;
  int ob, bn;
  if (task_override >= 0) {
    ob = task_override >> 4;
    bn = task_override & 15;
  } else if (S.fixed_obj >= 0) {
    ob = S.fixed_obj;
    bn = S.fixed_bin;
  } else if (!ok) {  // (the reference raised before its task draw)
    ob = EPI(EPI_OBJ);
    bn = EPI(EPI_BIN);
  } else {
    const int idx = pcg_integers(r, has32, buf32, S.ntask);
    ob = S.task_obj[idx];
    bn = S.task_bin[idx];
  }
  S.rng[4 * (size_t)i] = r.shi;
  S.rng[4 * (size_t)i + 1] = r.slo;
  EPI(EPI_RNG_HAS32) = has32;
  S.rng32[i] = buf32;
  EPI(EPI_OBJ) = ob;
  EPI(EPI_BIN) = bn;
  V3 cx;
  M3 cR;
  camera_pose(MMX_CAM_OVERHEAD, hx, hand_R(E), cx, cR);
  float kp[2];
  project(obj_pos(E, ob), cx, cR, MMX_cam_fovy[MMX_CAM_OVERHEAD], kp);
  EPF(EPF_TGTKP) = kp[0]; EPF(EPF_TGTKP + 1) = kp[1];
  project(bin_pos(bn), cx, cR, MMX_cam_fovy[MMX_CAM_OVERHEAD], kp);
  EPF(EPF_TGTKP + 2) = kp[0]; EPF(EPF_TGTKP + 3) = kp[1];
  // FSM expert for this episode's task (scripts/generate_dataset.py:112-117)
  EPI(EPI_FSM_STATE) = 0;
  EPI(EPI_FSM_TASKIDX) = 0;
  EPI(EPI_FSM_SETTLE) = 0;
  EPI(EPI_FSM_GRIP) = 1;
  EPI(EPI_FSM_HASTGT) = 0;
  EPI(EPI_PHASES) = 1;  // IDLE
  EPI(EPI_EPISODES) += 1;
  obs_lane0(S, i, E);
}

// the target cube inside the target bin (the success test of gym_env.py:436-447)
DEV bool in_target_bin(const MMXState& S, int i, const EnvSh& E) {
  const V3 o = obj_pos(E, EPI(EPI_OBJ)), b = bin_pos(EPI(EPI_BIN));
  return sqrtf((o.x - b.x) * (o.x - b.x) + (o.y - b.y) * (o.y - b.y)) < 0.05f && o.z < b.z + 0.06f;
}

// reward (gym_env.py:352-470); returns reward, sets success (staged: all HWM >= 0.9)
DEV float reward_lane0(const MMXState& S, int i, const EnvSh& E, bool robot_obstacle, int& success) {
  const int ob = EPI(EPI_OBJ), bn = EPI(EPI_BIN);
  const V3 o = obj_pos(E, ob), b = bin_pos(bn), ee = hand_pos(E);
  const float xy = sqrtf((o.x - b.x) * (o.x - b.x) + (o.y - b.y) * (o.y - b.y));
  const bool succ = xy < 0.05f && o.z < b.z + 0.06f;
  if (S.reward_type == 1) {
    success = succ;
    return succ ? 1.f : 0.f;
  }
  if (S.reward_type == 2) {
    const float DM = 0.5f, GZ = 0.35f, LZ = 0.42f;
    int fl = EPI(EPI_FLAGS);
    const bool closed = E.ctrl[7] == 0.f;
    if (!(fl & FLAG_GRASPED) && o.z > GZ && closed) fl |= FLAG_GRASPED;
    if (!(fl & FLAG_LIFTED) && o.z > LZ && closed) fl |= FLAG_LIFTED;
    if (!(fl & FLAG_ABOVE) && (fl & FLAG_LIFTED) && xy < 0.06f) fl |= FLAG_ABOVE;
    if (!(fl & FLAG_PLACED) && succ) fl |= FLAG_PLACED;
    float rr[5];
    rr[0] = (fl & FLAG_GRASPED) ? 1.f : 1.f - fminf(norm(ee - o) / DM, 1.f);
    rr[1] = !(fl & FLAG_GRASPED) ? 0.f : ((fl & FLAG_LIFTED) ? 1.f : fmaxf(0.f, fminf((o.z - 0.30f) / (LZ - 0.30f), 1.f)));
    rr[2] = !(fl & FLAG_LIFTED) ? 0.f : ((fl & FLAG_ABOVE) ? 1.f : 1.f - fminf(xy / DM, 1.f));
    rr[3] = !(fl & FLAG_ABOVE) ? 0.f : ((fl & FLAG_PLACED) ? 1.f : 1.f - fmaxf(0.f, fminf((o.z - b.z) / 0.25f, 1.f)));
    const V3 ip = V3{EPF(EPF_TINIT + 9), EPF(EPF_TINIT + 10), EPF(EPF_TINIT + 11)};
    rr[4] = !(fl & FLAG_PLACED) ? 0.f : 1.f - fminf(norm(ee - ip) / DM, 1.f);
    fl |= FLAG_HWM_VALID;
    EPI(EPI_FLAGS) = fl;
    float sum = 0.f;
    bool all = true;
#pragma unroll
    for (int k = 0; k < 5; k++) {
      const float h = fmaxf(EPF(EPF_HWM + k), rr[k]);
      EPF(EPF_HWM + k) = h;
      sum += h;
      all &= h >= 0.90f;
    }
    if (robot_obstacle) {
      success = 1;
      return -1.f;
    }
    success = all;
    return sum / 5.f;
  }
  float rew = -norm(ee - o);
  if (o.z > 0.30f) rew += 2.f - norm(o - b);
  if (succ) rew += 10.f;
  success = succ;
  return rew;
}

// FSM expert plan(n) (pick_and_place.py:167-277) -> abs_pos action (generate_dataset.py:142-148).
// ee / object positions come from the last position stage (consistent after mj_forward).
// PickAndPlaceTask.plan(n) (pick_and_place.py:167-277) in branch-free form: every transition
// condition is evaluated, then each FSM field takes its new value through selects.  (Two
// switch-statement forms of this function, called from one-lane-per-env divergent code, were
// miscompiled: the LOWER_TO_BIN target's z and then the emitted action's z came out wrong.)
DEV void expert_plan(const MMXState& S, int i, V3 o, V3 ee, int n, float* act4) {
  const int s = EPI(EPI_FSM_STATE), ti = EPI(EPI_FSM_TASKIDX), settle = EPI(EPI_FSM_SETTLE);
  const int grip = EPI(EPI_FSM_GRIP), has = EPI(EPI_FSM_HASTGT);
  const V3 t = V3{EPF(EPF_FSM_TARGET), EPF(EPF_FSM_TARGET + 1), EPF(EPF_FSM_TARGET + 2)};
  const V3 te = V3{EPF(EPF_FSM_TRANSIT), EPF(EPF_FSM_TRANSIT + 1), EPF(EPF_FSM_TRANSIT + 2)};
  const V3 b = bin_pos(EPI(EPI_BIN));
  const bool r = norm(ee - t) < 0.02f;  // controller.reached (controller.py:139-145)
  const int sn = settle - n;
  const bool idle_done = s == 0 && ti >= 1;  // single-task FSM: one pick and place, then DONE
  const bool go1 = s == 0 && ti < 1;          // IDLE -> PRE_GRASP
  const bool go2 = s == 1 && r;               // PRE_GRASP -> GRASP
  const bool go3 = s == 2 && r;               // GRASP -> CLOSE_GRIPPER
  const bool go4 = s == 3 && sn <= 0;         // CLOSE_GRIPPER -> LIFT
  const bool go5 = s == 4 && r;               // LIFT -> MOVE_TO_BIN
  const V3 diff = te - t;                     // MOVE_TO_BIN: advance 0.001 n toward the transit end
  const float dist = norm(diff), step = 0.001f * n;
  const V3 tmove = dist > step ? t + diff * (step / dist) : te;
  const bool go6 = s == 5 && dist <= 0.02f;   // (pre-move distance) -> SETTLE_AT_BIN
  const bool go7 = s == 6 && sn <= 0;         // SETTLE_AT_BIN -> LOWER_TO_BIN
  const bool go8 = s == 7 && r;               // LOWER_TO_BIN -> RELEASE
  const bool go9 = s == 8 && sn <= 0;         // RELEASE -> RETREAT
  const bool go0 = s == 9 && r;               // RETREAT -> IDLE (next task)
  float tx = t.x, ty = t.y, tz = t.z;
  tx = go1 || go2 || go4 ? o.x : tx;
  ty = go1 || go2 || go4 ? o.y : ty;
  tz = go1 ? 0.44f : (go2 ? 0.36f : (go4 ? 0.55f : tz));
  tx = s == 5 ? tmove.x : tx;
  ty = s == 5 ? tmove.y : ty;
  tz = s == 5 ? tmove.z : tz;
  tx = go7 ? b.x : (go9 ? 0.f : tx);
  ty = go7 ? b.y : (go9 ? 0.3f : ty);
  tz = go7 ? 0.45f : (go9 ? 0.55f : tz);
  const int ns = idle_done ? 10 : go1 ? 1 : go2 ? 2 : go3 ? 3 : go4 ? 4 : go5 ? 5 : go6 ? 6 : go7 ? 7
               : go8 ? 8 : go9 ? 9 : go0 ? 0 : s;
  int nset = (s == 3 || s == 6 || s == 8) ? sn : settle;
  nset = go3 || go8 ? 150 : (go6 ? 100 : nset);
  const int ng = go1 || go8 ? 1 : (go3 ? 0 : grip);
  const int nhas = go1 ? 1 : has;
  EPI(EPI_FSM_STATE) = ns; EPI(EPI_FSM_TASKIDX) = go0 ? ti + 1 : ti; EPI(EPI_FSM_SETTLE) = nset;
  EPI(EPI_PHASES) |= 1 << ns;
  EPI(EPI_FSM_GRIP) = ng; EPI(EPI_FSM_HASTGT) = nhas;
  EPF(EPF_FSM_TARGET) = tx; EPF(EPF_FSM_TARGET + 1) = ty; EPF(EPF_FSM_TARGET + 2) = tz;
  if (go5) {
    EPF(EPF_FSM_TRANSIT) = b.x; EPF(EPF_FSM_TRANSIT + 1) = b.y; EPF(EPF_FSM_TRANSIT + 2) = 0.55f;
  }
  // before the first plan the reference has no target and commands the current EE position
  act4[0] = nhas ? tx : ee.x; act4[1] = nhas ? ty : ee.y; act4[2] = nhas ? tz : ee.z;
  act4[3] = ng ? 1.f : 0.f;
}

// decode_action (gym_env.py:252-281) + gripper command (gym_env.py:550-553)
DEV void decode_lane0(const MMXState& S, int i, EnvSh& E, const float* a) {
  V3 p = V3{a[0], a[1], a[2]};
  float g;
  switch (S.action_mode) {
    case 0: g = a[3]; break;
    case 1: g = a[7]; break;
    case 2: g = a[9]; break;
    default: {
      float R[9];
#pragma unroll
      for (int k = 0; k < 9; k++) R[k] = EPF(EPF_TINIT + k);
      const V3 t = V3{EPF(EPF_TINIT + 9), EPF(EPF_TINIT + 10), EPF(EPF_TINIT + 11)};
      p = V3{R[0] * a[0] + R[1] * a[1] + R[2] * a[2] + t.x, R[3] * a[0] + R[4] * a[1] + R[5] * a[2] + t.y,
             R[6] * a[0] + R[7] * a[1] + R[8] * a[2] + t.z};
      g = S.action_mode == 3 ? a[7] : a[9];
    }
  }
  E.target[0] = p.x; E.target[1] = p.y; E.target[2] = p.z; E.target[3] = g;
  E.ctrl[7] = g > 0.5f ? 255.f : 0.f;
}

// ============================================================================ record I/O
DEV void load_env(const MMXState& S, int i, EnvSh& E) {
  if (LANE < 30) E.qpos[LANE] = S.qpos[(size_t)i * 30 + LANE];
  if (LANE < 27) {
    E.qvel[LANE] = S.qvel[(size_t)i * 27 + LANE];
    E.x[LANE] = S.qacc_ws[(size_t)i * 27 + LANE];
  }
  if (LANE < 8) E.ctrl[LANE] = S.ctrl[(size_t)i * 8 + LANE];
  if (LANE < KIN_N) kin_ref(E, LANE) = S.kin[(size_t)i * KIN_N + LANE];
  if (LANE < 4) E.target[LANE] = S.target[(size_t)i * 4 + LANE];
  if (LANE < STAT_N) E.stats[LANE] = S.stats[(size_t)i * STAT_N + LANE];
  if (LANE == 0) {
    E.ovf = S.efc_ovf + (size_t)i * MMX_OVF_F;
    E.flags = 0;
    E.ncon = 0;
    E.nefc = 0;
    E.nefc_mj = 0;
    E.ncand = -1;  // positions come from the record: rebuild the broadphase list
  }
  SYNC();
}
DEV void store_env(const MMXState& S, int i, const EnvSh& E) {
  SYNC();
  if (LANE < 30) S.qpos[(size_t)i * 30 + LANE] = E.qpos[LANE];
  if (LANE < 27) {
    S.qvel[(size_t)i * 27 + LANE] = E.qvel[LANE];
    S.qacc_ws[(size_t)i * 27 + LANE] = E.x[LANE];
  }
  if (LANE < 8) S.ctrl[(size_t)i * 8 + LANE] = E.ctrl[LANE];
  if (LANE < KIN_N) S.kin[(size_t)i * KIN_N + LANE] = kin_get(E, LANE);
  if (LANE < 4) S.target[(size_t)i * 4 + LANE] = E.target[LANE];
  if (LANE < STAT_N) S.stats[(size_t)i * STAT_N + LANE] = E.stats[LANE];
  if (S.rpose)  // body poses for the camera renderer (mmx_render.hip)
    for (int k = LANE; k < NSLOT * 12; k += WG) {
      const int sl = k / 12, c = k % 12;
      S.rpose[(size_t)i * NSLOT * 12 + k] = c < 9 ? E.bR[sl][c] : E.bx[sl][c - 9];
    }
}
DEV void store_obs(const MMXState& S, int i, const EnvSh& E) {
  SYNC();
  for (int k = LANE; k < MMX_NOBS; k += WG) S.obs[(size_t)i * MMX_NOBS + k] = obs_of(E)[k];
}
