// The 128-row step kernels (mmx_step.inc at its default layout: twelve envs per CU; with them the
// one-substep kernel of the physics harness) and every kernel that exists once, whatever the layout:
// forward, reset, the expert's loops, the reward harness, the episode queue and the dispatch order, with
// their launchers.  They use the 128-row LDS record of the include; mmx_step_l192.hip builds the step
// kernels and the one-substep kernel a second time at 192 rows.
#include "mmx_step.inc"

// mj_forward position stage only (kinematics -> IK cache) + observation refresh
extern "C" __global__ void __launch_bounds__(WG) mmx_forward_kernel(MMXState S) {
  EnvSh& E = g_E;
  const int i = blockIdx.x;
  if (i >= S.N) return;
  load_env(S, i, E);
  if (LANE == 0) {
    kinematics_lane0(E);
    obs_lane0(S, i, E);
  }
  store_env(S, i, E);
  store_obs(S, i, E);
}

extern "C" __global__ void __launch_bounds__(WG) mmx_reset_kernel(MMXState S, const unsigned char* mask, const int* task) {
  EnvSh& E = g_E;
  const int i = blockIdx.x;
  if (i >= S.N) return;
  if (mask && !mask[i]) return;
  load_env(S, i, E);
  if (LANE == 0) {
    EPI(EPI_ERROR) = 0;
    reset_lane0(S, i, E, task ? task[i] : -1);
    S.done[3 * (size_t)i] = 0;
    S.done[3 * (size_t)i + 1] = 0;
    S.done[3 * (size_t)i + 2] = 0;
  }
  store_env(S, i, E);
  store_obs(S, i, E);
}

// Per-physics-step expert loop (main.py:65-91, tests/test_pick_and_place.py:147-166): n x
// (PickAndPlaceTask.update() = plan(1) + _actuate() (pick_and_place.py:279-304) ; mj_step).  plan
// reads data.xpos as the previous mj_step left it: the hand pose and cube positions of
// the last position stage (the kin cache), not the integrated qpos.  No gym bookkeeping.
extern "C" __global__ void __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(2, 2)))
mmx_expert_physics_kernel(MMXState S, int n) {
  EnvSh& E = g_E;
  const int i = blockIdx.x;
  if (i >= S.N) return;
  load_env(S, i, E);
  for (int k = 0; k < n; k++) {
    if (LANE == 0) {
      float act[4];
      const int ob = EPI(EPI_OBJ);
      expert_plan(S, i, V3{E.bx[11 + ob][0], E.bx[11 + ob][1], E.bx[11 + ob][2]}, hand_pos(E), 1, act);
      // _actuate: gripper open / closed, then IK toward the target once there is one
      E.ctrl[7] = EPI(EPI_FSM_GRIP) ? 255.f : 0.f;
      E.target[0] = EPF(EPF_FSM_TARGET);
      E.target[1] = EPF(EPF_FSM_TARGET + 1);
      E.target[2] = EPF(EPF_FSM_TARGET + 2);
      E.target[3] = EPI(EPI_FSM_HASTGT) ? act[3] : -1.f;  // < 0: no target yet, no IK
    }
    SYNC();
    if (E.target[3] >= 0.f) ik_wave(E);
    SYNC();
    mj_step_wave(S.solver_max_iter, S.solver_tol, E, k == n - 1 ? contacts_dst(S, i) : nullptr);
  }
  if (LANE == 0) fold_flags(S, i, E);
  store_env(S, i, E);
}

// Contact forces of the current state (mmx_contact_forces; the reference reads them after env.step(), whose last
// call is mj_forward, gym_env.py:560): the forward part of mj_step_wave -- kinematics, dynamics, collision, the
// row build and the Newton solve from qacc_warmstart, no integrate_wave -- then MuJoCo's mj_contactForce /
// mju_decodePyramid on the solve, the per-body wrenches and the fingers' grip force.  A pass of its own: it
// reads the env record, writes only the arrays of F and works in F's overflow block, never the sim's (store_env
// is not called: qacc_warmstart, contacts, stats and the step kernels' broadphase list and axis cache stay).
//
// The decode: newton_wave overwrites the rows' aref (slot 15) and D, so both are taken into registers before
// the solve and the basis-row residuals r = J x - aref are formed again afterwards from the rows' J, which the
// solver leaves alone.  Edge e of a basis row k >= 1 is a_e r_n + b_e r_k exactly as the solver forms it
// (edge_coef, quad_first); its force is f_e = -D e where e < 0, else 0.  A contact's four basis rows sit in one
// DPP quad: fn = the quad's sum of f_e, component k = mu_k (f_k+ - f_k-), no LDS traffic; the quad's first lane
// then leaves (fn, t1, t2, torsion) in the scratch region at the row's index, where the contact's lane (lane c:
// contact c) finds it through the same type-ordered row map make_constraints_wave laid out.
// Every sum has a fixed order (a body's lane loops over the contacts by index) and there are no atomics.
DEV int force_body(int l) { return l < 10 ? l + 2 : l + 6; }  // 13 moving bodies: 2..11, then the cubes 16..18
#define FRC_CON_AT MMX_MAXEFC  // per-contact (force 3, torque 3, position 3, bodies) records behind the row forces
#define FRC_CON_W 12
static_assert(FRC_CON_AT + MMX_MAXCON * FRC_CON_W <= SCR_FLOATS, "the force pass's scratch exceeds the scratch region");
extern "C" __global__ void __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(2, 2)))
mmx_contact_force_kernel(MMXState S, MMXForce F) {
  EnvSh& E = g_E;
  const int i = blockIdx.x;
  if (i >= S.N) return;
  load_env(S, i, E);
  if (LANE == 0) E.ovf = F.ovf + (size_t)i * MMX_OVF_F;
  SYNC();
  kinematics_wave(E);
  dynamics_wave(E);
  collide_wave(E, false);
  store_contacts(F.contact + (size_t)i * MMX_MAXCON * CON_F, E);
  const int ncon = E.ncon;
  CReg own;  // the lane's contact (lane c: contact c), before the row build reuses the scratch that holds it
#pragma unroll
  for (int k = 0; k < CL_F; k++) own.v[k] = LANE < ncon ? crec(E, LANE)[k] : 0.f;
  float mu[RPL];
  make_constraints_wave(E, mu);
  const int nefc = E.nefc, nsingle = E.nsingle;
  float aref[RPL], dd[RPL];
#pragma unroll
  for (int q = 0; q < RPL; q++) {
    const int r = LANE + WG * q;
    aref[q] = 0.f;
    dd[q] = 0.f;
    if (WG * q >= nefc) continue;  // uniform: the slice holds no row
    if (r < nefc) {
      aref[q] = jget(E, r, 15);
      dd[q] = dget(E, r);
    }
  }
  float resid = 0.f;
  int exit = 0;
  const int it = newton_wave(E, S.solver_max_iter, S.solver_tol, resid, exit, mu);
  if (LANE < 27) F.qacc[(size_t)i * 27 + LANE] = E.x[LANE];
  // the rows' forces: per slice the quad's (fn, t1, t2, torsion), held by every lane of the quad
  ovf_fence(nefc);
  float cf[RPL][4];
#pragma unroll
  for (int q = 0; q < RPL; q++) {
    const int r = LANE + WG * q;
#pragma unroll
    for (int k = 0; k < 4; k++) cf[q][k] = 0.f;
    if (WG * q >= nefc) continue;  // uniform
    const float rr = r < nefc ? row_dot16(E, r, E.x) - aref[q] : 0.f;
    const float rn = quad_first(rr);
    const EdgeCoef ec = edge_coef(r, nefc, nsingle, r < nefc ? mu[q] : 0.f);
    const float e0 = fmaf(ec.a0, rn, ec.b0 * rr), e1 = fmaf(ec.a1, rn, ec.b1 * rr);
    const bool contact_row = r >= nsingle;  // (single rows: the equality and the limits, no contact's force)
    const float f0 = contact_row && e0 < 0.f ? -dd[q] * e0 : 0.f, f1 = contact_row && e1 < 0.f ? -dd[q] * e1 : 0.f;
    const float tk = ec.b0 * (f0 - f1);  // mu_k (f_k+ - f_k-); b0 = mu_k on a basis row with edges
    cf[q][0] = quad_sum(f0 + f1);
    cf[q][1] = dpp_f<0x55>(tk);  // quad_perm [1,1,1,1]
    cf[q][2] = dpp_f<0xAA>(tk);  // quad_perm [2,2,2,2]
    cf[q][3] = dpp_f<0xFF>(tk);  // quad_perm [3,3,3,3]
  }
  SYNC();  // every lane has read its rows: the scratch region is free
  float* scr = scr_of(E);
#pragma unroll
  for (int q = 0; q < RPL; q++) {
    const int r = LANE + WG * q;
    if (r < nefc && r >= nsingle && (r & 3) == 0) *reinterpret_cast<float4*>(scr + r) = make_float4(cf[q][0], cf[q][1], cf[q][2], cf[q][3]);
  }
  // the contact's first row, as make_constraints_wave placed it: by type, contacts of one type in lane order
  int tc = -1, brow = MMX_MAXEFC, b1 = 0, b2 = 0;
  if (LANE < ncon) {
    b1 = MMX_geom_body[con_g1(own)];
    b2 = MMX_geom_body[con_g2(own)];
    const int k1 = body_block(b1), k2 = body_block(b2);
    int rb0 = k1 >= 0 ? k1 : k2, rb1 = (k1 >= 0 && k2 >= 0 && k2 != k1) ? k2 : BLK_NONE;
    if (rb1 != BLK_NONE && rb1 < rb0) {
      const int t = rb0;
      rb0 = rb1;
      rb1 = t;
    }
    tc = row_type(rb0, rb1);
  }
#pragma unroll
  for (int t = 0; t < NTYPE; t++) {
    const unsigned long long m = __ballot(tc == t);
    if (tc == t)
      brow = E.tbase[t] + (t == 0 ? nsingle : 0) +
             4 * (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
  }
  SYNC();
  {
    float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (LANE < ncon && brow + 3 < nefc) c4 = *reinterpret_cast<const float4*>(scr + brow);  // (else: rows past MMX_MAXEFC)
    const V3 n = V3{own[CL_N], own[CL_N + 1], own[CL_N + 2]};
    const V3 t1 = contact_t1(n);
    const V3 f = n * c4.x + t1 * c4.y + cross(n, t1) * c4.z;
    float* o = F.force + ((size_t)i * MMX_MAXCON + LANE) * FRC_F;
    const bool live = LANE < ncon;
    o[0] = live ? c4.x : 0.f;
    o[1] = live ? f.x : 0.f;
    o[2] = live ? f.y : 0.f;
    o[3] = live ? f.z : 0.f;
    o[4] = live ? c4.w : 0.f;
    float* w = scr + FRC_CON_AT + FRC_CON_W * LANE;
    w[0] = f.x; w[1] = f.y; w[2] = f.z;
    w[3] = n.x * c4.w; w[4] = n.y * c4.w; w[5] = n.z * c4.w;
    w[6] = own[CL_POS]; w[7] = own[CL_POS + 1]; w[8] = own[CL_POS + 2];
    w[9] = c4.x;
    w[10] = __int_as_float(b1);
    w[11] = __int_as_float(b2);
  }
  SYNC();
  if (LANE < FRC_NBODY) {  // the body's lane adds its contacts' forces in index order
    const int b = force_body(LANE);
    const V3 x = body_x(E, b);
    V3 fs = V3{0.f, 0.f, 0.f}, ts = fs;
    for (int c = 0; c < ncon; c++) {
      const float* w = scr + FRC_CON_AT + FRC_CON_W * c;
      const int c1 = __float_as_int(w[10]), c2 = __float_as_int(w[11]);
      if (c1 != b && c2 != b) continue;
      const float sg = c2 == b ? 1.f : -1.f;  // the force acts on geom2's body, its opposite on geom1's
      const V3 f = V3{w[0], w[1], w[2]} * sg;
      fs = fs + f;
      ts = ts + cross(V3{w[6], w[7], w[8]} - x, f) + V3{w[3], w[4], w[5]} * sg;
    }
    float* o = F.wrench + ((size_t)i * FRC_NBODY + LANE) * 6;
    o[0] = fs.x; o[1] = fs.y; o[2] = fs.z;
    o[3] = ts.x; o[4] = ts.y; o[5] = ts.z;
  } else if (LANE < FRC_NBODY + 2) {  // the grip force: finger 10 / 11 against any cube
    const int b = 10 + LANE - FRC_NBODY;
    float s = 0.f;
    for (int c = 0; c < ncon; c++) {
      const float* w = scr + FRC_CON_AT + FRC_CON_W * c;
      const int c1 = __float_as_int(w[10]), c2 = __float_as_int(w[11]);
      if ((c1 == b && c2 >= MMX_BODY_OBJ_RED) || (c2 == b && c1 >= MMX_BODY_OBJ_RED)) s += w[9];
    }
    F.touch[2 * (size_t)i + LANE - FRC_NBODY] = s;
  } else if (LANE == FRC_NBODY + 2) {
    float* o = F.solve + (size_t)i * FRC_SOLVE_F;
    o[0] = (float)ncon;
    o[1] = (float)E.nefc_mj;
    o[2] = (float)it;
    o[3] = resid;
    o[4] = (float)exit;
    o[5] = (float)(E.flags & (SHF_CON_OVF | SHF_EFC_OVF));
  }
}

// Reward-layer parity harness (gym_env.py:341-470, 562-573): the reward of every env at the given
// object / EE positions and gripper command, with the step's contacts given as geom-id pairs (-1
// ends a list; robot x obstacle pairs are classified by the same geom classes as the collision
// scan).  Updates the sticky flags / high-water marks like a step; writes reward, reward
// components, terminated and success.
extern "C" __global__ void __launch_bounds__(WG) mmx_reward_kernel(MMXState S, const float* obj, const float* ee,
                                                                  const float* ctrl7, const int* pairs, int max_pairs) {
  EnvSh& E = g_E;
  const int i = blockIdx.x;
  if (i >= S.N || LANE != 0) return;
  const int ob = EPI(EPI_OBJ);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    E.qpos[9 + 7 * ob + k] = obj[3 * (size_t)i + k];
    kin_ref(E, KIN_HAND_POS + k) = ee[3 * (size_t)i + k];
  }
  E.ctrl[7] = ctrl7[i];
  bool ro = false;
  for (int p = 0; p < max_pairs; p++) {
    const int g1 = pairs[2 * ((size_t)i * max_pairs + p)], g2 = pairs[2 * ((size_t)i * max_pairs + p) + 1];
    if (g1 < 0 || g2 < 0 || g1 >= MMX_NGEOM || g2 >= MMX_NGEOM) break;
    const int c1 = MMX_geom_class[g1], c2 = MMX_geom_class[g2];
    ro |= (c1 == 1 && c2 == 2) || (c1 == 2 && c2 == 1);
  }
  int terminated, succ_flag;
  reward_outputs(S, i, E, ro, terminated, succ_flag);
  S.done[3 * (size_t)i] = terminated;
  S.done[3 * (size_t)i + 1] = 0;
  S.done[3 * (size_t)i + 2] = succ_flag;
}

// FSM expert plan(n) for every env -> abs_pos action [N][4] (one lane per env: tiny)
extern "C" __global__ void __launch_bounds__(WG) mmx_expert_kernel(MMXState S, int n, float* action) {
  const int i = blockIdx.x * WG + threadIdx.x;
  if (i >= S.N) return;
  const int ob = EPI(EPI_OBJ);
  const float* q = S.qpos + (size_t)i * 30;
  const float* kn = S.kin + (size_t)i * KIN_N;
  float a[4];
  expert_plan(S, i, V3{q[9 + 7 * ob], q[10 + 7 * ob], q[11 + 7 * ob]}, V3{kn[0], kn[1], kn[2]}, n, a);
  if (action)
    for (int k = 0; k < 4; k++) action[(size_t)i * 4 + k] = a[k];
}

// ============================================================================ episode queue
// Device-side slot reassignment of the dataset loop (scripts/generate_dataset.py:140-198 runs one
// episode per env; here E episodes stream through the N env slots, mmx_queue_advance).  One
// workgroup scans the slots in order and hands episodes next, next + 1, ... to the slots that need
// one (no episode yet, or their FSM reached DONE = state 10, pick_and_place.py:167-277), staging the
// reset: mask, task and the episode's PCG64(SeedSequence(seed_e)) state (generate_dataset.py:263-277).
// The slot -> episode order is the host loop's (finished slots in ascending order).
struct MMXQueue {
  int* slot;                      // [N] episode running in the slot, -1: none
  int* next;                      // [1] next episode to hand out
  int n_ep;                       // E
  const unsigned long long* rng;  // [E][4] initial PCG64 state per episode, or null (no reseed)
  const int* task;                // [E] obj << 4 | bin, -1: the env's own draw
};
#define QWG 1024
extern "C" __global__ void __launch_bounds__(QWG) mmx_queue_kernel(MMXState S, MMXQueue Q, unsigned char* mask, int* task,
                                                                  int* slot_out, int* fin_out) {
  __shared__ int scan[QWG];
  const int t = threadIdx.x, N = S.N;
  const int c = (N + QWG - 1) / QWG, s0 = min(N, t * c), s1 = min(N, s0 + c);  // contiguous slots per thread
  int cnt = 0;
  for (int s = s0; s < s1; s++) cnt += Q.slot[s] < 0 || S.epi[(size_t)s * EPI_N + EPI_FSM_STATE] == 10;
  scan[t] = cnt;
  __syncthreads();
  for (int off = 1; off < QWG; off <<= 1) {  // inclusive scan of the per-thread counts
    const int v = t >= off ? scan[t - off] : 0;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  const int base = *Q.next;
  int e = base + scan[t] - cnt;
  for (int s = s0; s < s1; s++) {
    const int cur = Q.slot[s];
    const bool ended = cur >= 0 && S.epi[(size_t)s * EPI_N + EPI_FSM_STATE] == 10;
    int now = cur;
    unsigned char m = 0;
    if (cur < 0 || ended) {
      now = e < Q.n_ep ? e : -1;
      if (now >= 0) {
        m = 1;
        task[s] = Q.task[now];
        if (Q.rng) {
#pragma unroll
          for (int k = 0; k < 4; k++) S.rng[4 * (size_t)s + k] = Q.rng[4 * (size_t)now + k];
          S.epi[(size_t)s * EPI_N + EPI_RNG_HAS32] = 0;
        }
      }
      e++;
      Q.slot[s] = now;
    }
    mask[s] = m;
    if (slot_out) slot_out[s] = now;
    if (fin_out) fin_out[s] = ended ? cur : -1;
  }
  __syncthreads();
  if (t == 0) *Q.next = min(Q.n_ep, base + scan[QWG - 1]);
}

// Dispatch order of an env range for the step kernel, longest first.  An env step's cycles follow its
// FSM phase (profiles/r06_fsm_profile.json, cycles per env step at twelve per CU): lift / move to bin /
// lower to bin ~2.5 M, close gripper / settle ~2.2 M, release / retreat ~1.7 M, the rest ~1.4-1.5 M.  A counting
// sort over those four classes (refined by rows, below) puts the long ones at the front of order[],
// so the launch's last workgroups are short ones (C3 +2.0 %, C5 +3.8 %).  One workgroup of any size (a single
// wave beside running step launches: it then fits a CU the step kernel fills); the order within a
// class is whatever the atomics give (the envs are independent: results do not depend on it).
DEV int step_cost_class(int fsm_state) {
  switch (fsm_state) {
    case 4: case 5: case 7: return 0;  // lift, move to bin, lower to bin (the object held)
    case 3: case 6: return 1;          // close gripper, settle at bin
    case 8: case 9: return 2;          // release, retreat
    default: return 3;
  }
}
// the sort key: the phase class first, then within a class the env's constraint rows of its last
// substep (MuJoCo's count, EPI_NEFC) in 32-row steps, more rows first (C5 +1.0 %, C3 unchanged; rows
// alone: C5 +0.5 %, C3 -1.1 %: a fused launch's steps follow the phase more than the last rows)
#define ORD_NB 24
DEV int step_order_bucket(const MMXState& S, int i) {
  const int c = step_cost_class(S.epi[(size_t)i * EPI_N + EPI_FSM_STATE]);
  return 6 * c + 5 - min(5, S.epi[(size_t)i * EPI_N + EPI_NEFC] >> 5);
}
extern "C" __global__ void __launch_bounds__(1024) mmx_order_kernel(MMXState S, int base, int count, int* order) {
  __shared__ int cnt[ORD_NB], off[ORD_NB];
  if (threadIdx.x < ORD_NB) cnt[threadIdx.x] = 0;
  __syncthreads();
  for (int k = threadIdx.x; k < count; k += blockDim.x) atomicAdd(&cnt[step_order_bucket(S, base + k)], 1);
  __syncthreads();
  if (threadIdx.x == 0)
    for (int b = 0, o = 0; b < ORD_NB; b++) off[b] = o, o += cnt[b];
  __syncthreads();
  for (int k = threadIdx.x; k < count; k += blockDim.x) {
    const int i = base + k;
    order[atomicAdd(&off[step_order_bucket(S, i)], 1)] = i;
  }
}

// =========================================================================== host launchers
// threads: 1024 when the launch has the GPU to itself, 64 beside other streams' step launches (a
// 1,024-lane workgroup waited ~0.35 ms for a CU to drain there: profiles/archive/r05_c3_kernel_stats.csv)
extern "C" hipError_t mmx_launch_order(const MMXState* S, int base, int count, int* order, int threads, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  if (threads != 64 && threads != 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mmx_order_kernel, dim3(1), dim3(threads), 0, st, *S, base, count, order);
  return hipGetLastError();
}
extern "C" hipError_t mmx_launch_queue(const MMXState* S, int* slot, int* next, int n_ep, const unsigned long long* rng,
                                       const int* qtask, unsigned char* mask, int* task, int* slot_out, int* fin_out,
                                       hipStream_t st) {
  const MMXQueue Q{slot, next, n_ep, rng, qtask};
  hipLaunchKernelGGL(mmx_queue_kernel, dim3(1), dim3(QWG), 0, st, *S, Q, mask, task, slot_out, fin_out);
  return hipGetLastError();
}
extern "C" hipError_t mmx_launch_reset(const MMXState* S, const unsigned char* mask, const int* task, hipStream_t st) {
  hipLaunchKernelGGL(mmx_reset_kernel, dim3(S->N), dim3(WG), 0, st, *S, mask, task);
  return hipGetLastError();
}
extern "C" hipError_t mmx_launch_expert(const MMXState* S, int n, float* action, hipStream_t st) {
  hipLaunchKernelGGL(mmx_expert_kernel, dim3((S->N + WG - 1) / WG), dim3(WG), 0, st, *S, n, action);
  return hipGetLastError();
}
extern "C" hipError_t mmx_launch_expert_physics(const MMXState* S, int n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(mmx_expert_physics_kernel, dim3(S->N), dim3(WG), 0, st, *S, n);
  return hipGetLastError();
}
extern "C" hipError_t mmx_launch_contact_force(const MMXState* S, const MMXForce* F, hipStream_t st) {
  hipLaunchKernelGGL(mmx_contact_force_kernel, dim3(S->N), dim3(WG), 0, st, *S, *F);
  return hipGetLastError();
}
extern "C" hipError_t mmx_launch_reward(const MMXState* S, const float* obj, const float* ee, const float* ctrl7,
                                        const int* pairs, int max_pairs, hipStream_t st) {
  hipLaunchKernelGGL(mmx_reward_kernel, dim3(S->N), dim3(WG), 0, st, *S, obj, ee, ctrl7, pairs, max_pairs);
  return hipGetLastError();
}
extern "C" hipError_t mmx_launch_forward(const MMXState* S, hipStream_t st) {
  hipLaunchKernelGGL(mmx_forward_kernel, dim3(S->N), dim3(WG), 0, st, *S);
  return hipGetLastError();
}
#ifdef MMX_PHASE_CLOCK
// the profile build's per-FSM-state sums of the 128-row step kernel (g_fsm_prof, mmx_step_kernels.inc)
extern "C" hipError_t mmx_fsm_profile(double* out, int reset) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fsm_prof), sizeof(g_fsm_prof));
  if (e == hipSuccess && reset) {
    static double z[11 * FSMP_N];
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_fsm_prof), z, sizeof(z));
  }
  return e;
}
extern "C" int mmx_fsm_profile_fields() { return FSMP_N; }
#endif
