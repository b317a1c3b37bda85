// Part 4 of mmx_step.inc (an ordered fragment, included there and nowhere else): the constraint rows.
// make_constraints_wave turns the finger equality, the joint limits and the sorted contacts (four basis rows
// each) into rows grouped by block-pair type, in LDS and, past MMX_LDSEFC rows, in the env's overflow record,
// and hands the rows' mu to the solver in registers.  Relies on the lds part (the contact record in
// registers, the row accessors, the dof-block tables, ovf_fence) and on the contacts the collision part left.
// ============================================================================ constraints (wave)
// Soft-constraint reference terms of a row: K, B from solref, impedance from solimp (MuJoCo
// mj_makeImpedance); D = 1 / R with R = (1 - imp) / imp * diag.
DEV void row_ref(const float* solref, const float* solimp, float pos, float& imp_ratio, float& kid, float& B) {
  const float imp = impedance(solimp, pos);
  const float dmax = fminf(fmaxf(solimp[1], 1e-4f), 0.9999f);
  const float tc = fmaxf(solref[0], 2.f * kDt), dr = solref[1];
  const float K = 1.f / (dmax * dmax * tc * tc * dr * dr);
  B = 2.f / (dmax * tc);
  imp_ratio = (1.f - imp) / imp;
  kid = K * imp * pos;
}
DEV void store_row(EnvSh& E, int row, const float* jv, int hdr, float vel, float imp_ratio, float kid, float B,
                   float diag) {
  const float aref = -B * vel - kid;  // slot 15
  if (row < MMX_LDSEFC) {
#pragma unroll
    for (int q = 0; q < 3; q++)
      *reinterpret_cast<float4*>(E.J[q][row]) = make_float4(jv[4 * q], jv[4 * q + 1], jv[4 * q + 2], jv[4 * q + 3]);
    *reinterpret_cast<float4*>(E.J[3][row]) = make_float4(jv[12], jv[13], jv[14], aref);
  } else {
    float4* Jr = reinterpret_cast<float4*>(ovf_j(E, row));
#pragma unroll
    for (int q = 0; q < 3; q++) Jr[q] = make_float4(jv[4 * q], jv[4 * q + 1], jv[4 * q + 2], jv[4 * q + 3]);
    Jr[3] = make_float4(jv[12], jv[13], jv[14], aref);
  }
  hdr_set(E, row, hdr);
  dset(E, row, 1.f / fmaxf(imp_ratio * diag, 1e-15f));
}

// A contact's mixed parameters (MuJoCo: friction and condim the max of the two geoms', solref /
// solimp their mean) and reference terms: computed by each of its basis rows' lanes from the
// 9-float LDS record (the rows of one contact are built by up to four lanes; the same inputs and
// arithmetic give each the same values)
struct ConPar {
  int dim;
  float mu0, mu1, kid, B, idiag;
};
template <class R>
DEV ConPar contact_params(const R& cc) {
  const int g1 = con_g1(cc), g2 = con_g2(cc);
  ConPar P;
  P.dim = max(MMX_geom_condim[g1], MMX_geom_condim[g2]);
  P.mu0 = fmaxf(MMX_geom_friction[3 * g1], MMX_geom_friction[3 * g2]);
  P.mu1 = fmaxf(MMX_geom_friction[3 * g1 + 1], MMX_geom_friction[3 * g2 + 1]);
  float solref[2], solimp[5];
#pragma unroll
  for (int k = 0; k < 2; k++) solref[k] = 0.5f * (MMX_geom_solref[2 * g1 + k] + MMX_geom_solref[2 * g2 + k]);
#pragma unroll
  for (int k = 0; k < 5; k++) solimp[k] = 0.5f * (MMX_geom_solimp[5 * g1 + k] + MMX_geom_solimp[5 * g2 + k]);
  float impr;
  row_ref(solref, solimp, cc[CL_DIST], impr, P.kid, P.B);
  const int b1 = MMX_geom_body[g1], b2 = MMX_geom_body[g2];
  const float tran = MMX_body_invweight0[2 * b1] + MMX_body_invweight0[2 * b2];
  const float it = impr * tran;  // (the pyramid's common R needs only the translational invweight)
  // pyramidal cone: one R for every edge, A_hat = 2 mu0^2 (tran + mu0^2 tran) / impratio (impratio
  // = 1), R = (1 - d) / d A_hat; pinned by the closed-form scenes of tests/test_physics_kat.py
  P.idiag = P.dim > 1 ? 2.f * P.mu0 * P.mu0 * (it + P.mu0 * P.mu0 * it) : it;
  return P;
}
DEV V3 contact_t1(V3 n) {  // mju_makeFrame's first tangent
  const V3 y = (n.y < 0.5f && n.y > -0.5f) ? V3{0.f, 1.f, 0.f} : V3{0.f, 0.f, 1.f};
  return normalize(y - n * dot(n, y));
}

// Basis row rr of contact c, built straight into block format: rr 0 = normal, 1 / 2 = tangents
// t1 / t2 (mju_makeFrame), 3 = rotation about the normal (torsion, condim 4).  MuJoCo's pyramid
// edges of the contact are J_n +/- mu_k J_k (k = t1, t2 with the sliding mu, torsion with the
// torsional mu) and their aref = aref_n +/- mu_k aref_k with aref_k = -B J_k qvel (the position
// term belongs to the normal); the solver forms them from these rows.  An arm block entry is the
// motion subspace of dof d seen at the contact point, a cube block the free-body Jacobian.  Rows the
// contact's condim does not use are zero rows with D = 0.  Returns the row's mu (-1: no edges).
DEV float contact_row(EnvSh& E, int row, const CReg& cc, int rr, const ConPar& P) {
  const V3 p = V3{cc[CL_POS], cc[CL_POS + 1], cc[CL_POS + 2]};
  const V3 n = V3{cc[CL_N], cc[CL_N + 1], cc[CL_N + 2]};
  const int b1 = MMX_geom_body[con_g1(cc)], b2 = MMX_geom_body[con_g2(cc)];
  const int dim = P.dim;
  const bool used = rr == 0 || (rr < 3 && dim >= 3) || (rr == 3 && dim >= 4);
  const V3 t1 = contact_t1(n);
  const V3 u = rr == 0 ? n : (rr == 1 ? t1 : (rr == 2 ? cross(n, t1) : V3{0.f, 0.f, 0.f}));
  const V3 w = rr == 3 ? n : V3{0.f, 0.f, 0.f};
  const float idiag = P.idiag;  // impedance ratio x diagApprox
  const int k1 = body_block(b1), k2 = body_block(b2);
  int rb0 = k1 >= 0 ? k1 : k2, rb1 = (k1 >= 0 && k2 >= 0 && k2 != k1) ? k2 : BLK_NONE;
  if (rb1 != BLK_NONE && rb1 < rb0) {
    const int t = rb0;
    rb0 = rb1;
    rb1 = t;
  }
  // arm block: coefficient +1 / -1 / 0 of dof d from the two bodies' ancestor-dof masks
  const unsigned am1 = anc_mask(b1), am2 = anc_mask(b2);
  float vel = 0.f;
  float arm[9];
  // u . (v_d + w_d x p) + w . w_d = u . v_d + w_d . (p x u + w): one cross product per row
  const V3 pu = cross(p, u) + w;
#pragma unroll
  for (int d = 0; d < 9; d++) {  // body 2 counts +, body 1 counts -
    const float coef = (float)((int)((am2 >> d) & 1u) - (int)((am1 >> d) & 1u));
    const SV sd = load_S(E, d);
    arm[d] = coef * (dot(u, sd.v) + dot(sd.w, pu));
    vel = fmaf(arm[d], E.qvel[d], vel);
  }
  float cubeA[6], cubeB[6];  // blocks rb0 (when a cube) and rb1
  // each body's free-body columns (zero unless it is a cube), velocity summed in body order; block
  // A (rb0) is body 1's unless body 1 is not rb0
  float cvs[2][6];
#pragma unroll
  for (int side = 0; side < 2; side++) {
    const int b = side ? b2 : b1, blk = side ? k2 : k1;
#pragma unroll
    for (int j = 0; j < 6; j++) cvs[side][j] = 0.f;
    if (blk > 0) {
      const float sg = side ? 1.f : -1.f;
      const V3 x = body_x(E, b);
      const M3 R = body_R(E, b);
      cvs[side][0] = sg * u.x;
      cvs[side][1] = sg * u.y;
      cvs[side][2] = sg * u.z;
      const V3 ru = cross(p - x, u) + w;  // u . (r_k x (p - x)) + w . r_k = r_k . ((p - x) x u + w)
#pragma unroll
      for (int k = 0; k < 3; k++) cvs[side][3 + k] = sg * dot(col(R, k), ru);
      const int d0 = blk_d0(blk);
#pragma unroll
      for (int j = 0; j < 6; j++) vel = fmaf(cvs[side][j], E.qvel[d0 + j], vel);
    }
  }
  const bool swap = k1 != rb0;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    cubeA[j] = swap ? cvs[1][j] : cvs[0][j];
    cubeB[j] = swap ? cvs[0][j] : cvs[1][j];
  }
  float jv[16];
  const bool armrow = rb0 == 0;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const float va = j < 9 ? arm[j] : (j < 15 ? cubeB[j - 9] : 0.f);
    const float vc = j < 6 ? cubeA[j] : (j < 12 ? cubeB[j - 6] : 0.f);
    jv[j] = armrow ? va : vc;
  }
  store_row(E, row, jv, rb0 | (rb1 << 4), vel, 1.f, rr == 0 ? P.kid : 0.f, P.B, idiag);
  if (!used) dset(E, row, 0.f);  // (its J is zero as well: u = w = 0)
  return !used || rr == 0 ? (rr == 0 ? 0.f : -1.f) : (rr < 3 ? P.mu0 : P.mu1);
}

// Constraint rows in MuJoCo's order per lane scan: finger equality (lane 0), joint limits
// (lanes 0..8), contacts (lane c = contact c, 4 basis rows each).  Equality and limit rows are
// written by their lanes; contact rows are spread over all lanes through a row -> (contact, basis
// row) map.  Rows are grouped by block-pair type in aligned groups of 4 (type 0 starts with the
// equality / limit rows, padded with zero rows to a multiple of 4); the rows' mu (the solver's
// edge coefficients) go to the solver in registers (mu_out, the lane's rows LANE + 64 q).
DEV void make_constraints_wave(EnvSh& E, float* mu_out) {
  float* stats = E.stats;
  CLK_DECL;
  const float def_ref[2] = {0.02f, 1.0f};
  const float def_imp[5] = {0.9f, 0.95f, 0.001f, 0.5f, 2.0f};
  const int ncon = E.ncon;
  // the lane's own contact into registers (lane c: contact c): the rows overwrite the scratch region
  // that holds the contacts, and each row's lane reads its contact's fields from lane c (ds_bpermute)
  CReg own;
#pragma unroll
  for (int k = 0; k < CL_F; k++) own.v[k] = LANE < ncon ? crec(E, LANE)[k] : 0.f;
  // row -> (contact, basis row) map, -1 for the equality / limit / padding rows; it lives in the
  // rows' D (dset / dget), so the equality / limit rows (whose store_row writes D) are stored after
  // the contact rows
  auto rowmap_set = [&](int r, int m) { dset(E, r, __int_as_float(m)); };
  int nlim = 0, tc = -1, nedge = 0;
  bool lo_act = false, hi_act = false;
  if (LANE < 9) {
    const float q = E.qpos[LANE];
    lo_act = q - MMX_jnt_range[2 * LANE] < 0.f;
    hi_act = MMX_jnt_range[2 * LANE + 1] - q < 0.f;
    nlim = (int)lo_act + (int)hi_act;
  }
  if (LANE < ncon) {
    const int g1 = con_g1(own), g2 = con_g2(own);
    const int dim = max(MMX_geom_condim[g1], MMX_geom_condim[g2]);
    nedge = dim == 1 ? 1 : 2 * (dim - 1);
    const int k1 = body_block(MMX_geom_body[g1]), k2 = body_block(MMX_geom_body[g2]);
    int rb0 = k1 >= 0 ? k1 : k2, rb1 = (k1 >= 0 && k2 >= 0 && k2 != k1) ? k2 : BLK_NONE;
    if (rb1 != BLK_NONE && rb1 < rb0) {
      const int t = rb0;
      rb0 = rb1;
      rb1 = t;
    }
    tc = row_type(rb0, rb1);
  }
  // single rows (equality + limits), then per type the contact groups
  const int acnt = (LANE == 0 ? 1 : 0) + nlim;
  // acnt <= 3: its two bits as ballots give the exclusive prefix and the total without a scan
  const unsigned long long a0 = __ballot(acnt & 1), a1 = __ballot(acnt & 2);
  const int nsingle_raw = __popcll(a0) + 2 * __popcll(a1);
  const int arow = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(a0 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)a0, 0u)) +
                   2 * (int)__builtin_amdgcn_mbcnt_hi((unsigned)(a1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)a1, 0u));
  const int nsingle = (nsingle_raw + 3) & ~3;
  int brow = 0, base = 0;
  // per type: one ballot of the contacts (lanes) of that type; a lane's rows start at the type's
  // base plus 4 x the contacts of its type in lower lanes (mbcnt), so no prefix scans
#pragma unroll
  for (int t = 0; t < NTYPE; t++) {
    const unsigned long long m = __ballot(tc == t);
    const int first = base + (t == 0 ? nsingle : 0);  // type 0: the single rows come first
    if (tc == t) brow = first + 4 * (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    if (LANE == 0) E.tbase[t] = min(base, MMX_MAXEFC);
    base = first + 4 * __popcll(m);
  }
  const int total = base;
  const int nefc = min(total, MMX_MAXEFC);
  const int nefc_mj = nsingle_raw + __popcll(__ballot(nedge & 1)) + 2 * __popcll(__ballot(nedge & 2)) +
                      4 * __popcll(__ballot(nedge & 4));  // nedge <= 6
  if (LANE == 0) {
    E.tbase[NTYPE] = nefc;
    E.nefc = nefc;
    E.nefc_mj = nefc_mj;
    E.nsingle = nsingle;
    if (total > MMX_MAXEFC) E.flags |= SHF_EFC_OVF;
  }
  PROBE(3, stats, STAT_T_AUX0);
  if (LANE < 4 && nsingle_raw + LANE < nsingle) rowmap_set(nsingle_raw + LANE, -1);  // padding
  int row = arow;
  if (LANE == 0 && row < MMX_MAXEFC) rowmap_set(row++, -1);  // finger equality
  if (LANE < 9) {
#pragma unroll
    for (int side = 0; side < 2; side++)
      if ((side == 0 ? lo_act : hi_act) && row < MMX_MAXEFC) rowmap_set(row++, -1);  // joint limits
  }
  PROBE(3, stats, STAT_T_AUX1);
  // each contact's parameters computed once, by its lane, and read by its rows' lanes over ds_bpermute
  // (computing them per row measured -1.3 %, DESIGN §2)
  ConPar Pc{1, 0.f, 0.f, 0.f, 0.f, 1.f};
  if (LANE < ncon) Pc = contact_params(own);
  if (LANE < ncon) {  // the contact's 4 basis rows in the row -> (contact, basis row) map
#pragma unroll
    for (int rr = 0; rr < 4; rr++)
      if (brow + rr < MMX_MAXEFC) rowmap_set(brow + rr, LANE | (rr << 8));
  }
  ovf_fence(nefc);
  SYNC();
  PROBE(3, stats, STAT_T_AUX3);
  constexpr int RPB = (MMX_MAXEFC + WG - 1) / WG;
  float mu[RPB];
#pragma unroll
  for (int q = 0; q < RPB; q++) {
    const int r = LANE + WG * q;
    mu[q] = 0.f;
    if (WG * q >= nefc) continue;  // uniform: no row in this slice
    const int m = r < nefc ? __float_as_int(dget(E, r)) : -1;
    const int c = m >= 0 ? (m & 255) : 0;
    ConPar P;  // contact c's parameters from lane c (every lane takes part in the exchange)
    P.dim = __shfl(Pc.dim, c);
    P.mu0 = __shfl(Pc.mu0, c);
    P.mu1 = __shfl(Pc.mu1, c);
    P.kid = __shfl(Pc.kid, c);
    P.B = __shfl(Pc.B, c);
    P.idiag = __shfl(Pc.idiag, c);
    CReg cc;  // contact c's position, normal and geoms from lane c
    cc.v[CL_DIST] = 0.f;
#pragma unroll
    for (int k = CL_POS; k < CL_F; k++) cc.v[k] = __shfl(own.v[k], c);
    if (m >= 0) mu[q] = contact_row(E, r, cc, m >> 8, P);
  }
  row = arow;
  float jv[16];
  if (LANE == 0 && row < MMX_MAXEFC) {  // finger equality (panda.xml:261)
#pragma unroll
    for (int j = 0; j < 16; j++) jv[j] = j == 7 ? 1.f : (j == 8 ? -1.f : 0.f);
    float ir, kid, B;
    row_ref(MMX_eq_solref, MMX_eq_solimp, E.qpos[7] - E.qpos[8], ir, kid, B);
    store_row(E, row, jv, 0 | (BLK_NONE << 4), E.qvel[7] - E.qvel[8], ir, kid, B,
              MMX_dof_invweight0[7] + MMX_dof_invweight0[8]);
    row++;
  }
  if (LANE < 9) {  // joint limits (MuJoCo default solref / solimp)
    const float q = E.qpos[LANE];
#pragma unroll
    for (int side = 0; side < 2; side++) {
      const bool act = side == 0 ? lo_act : hi_act;
      if (act && row < MMX_MAXEFC) {
        const float sg = side == 0 ? 1.f : -1.f;
#pragma unroll
        for (int j = 0; j < 16; j++) jv[j] = j == LANE ? sg : 0.f;
        const float dist = side == 0 ? q - MMX_jnt_range[2 * LANE] : MMX_jnt_range[2 * LANE + 1] - q;
        float ir, kid, B;
        row_ref(def_ref, def_imp, dist, ir, kid, B);
        store_row(E, row, jv, 0 | (BLK_NONE << 4), sg * E.qvel[LANE], ir, kid, B, MMX_dof_invweight0[LANE]);
        row++;
      }
    }
  }
  if (LANE < 4 && nsingle_raw + LANE < nsingle) {  // zero padding rows (weight 0)
#pragma unroll
    for (int j = 0; j < 16; j++) jv[j] = 0.f;
    store_row(E, nsingle_raw + LANE, jv, 0 | (BLK_NONE << 4), 0.f, 1.f, 0.f, 0.f, 1.f);
    dset(E, nsingle_raw + LANE, 0.f);
  }
  ovf_fence(nefc);
  SYNC();  // every row is built; the rows' mu go to the solver in registers
#pragma unroll
  for (int q = 0; q < RPB; q++) mu_out[q] = mu[q];
  PROBE(3, stats, STAT_T_AUX2);
}
