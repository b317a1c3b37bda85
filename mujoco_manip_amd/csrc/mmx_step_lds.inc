// Part 1 of mmx_step.inc (an ordered fragment, included there and nowhere else): the env's LDS.  The contact
// record, EnvSh and its one instance g_E, the map of the scratch overlays (COL_*, SCR_*) with the static_asserts
// that keep them apart, the wave-delay hooks of the test builds (DELAY_HELPER / DELAY_ENV), the accessors of the
// rows, contacts, kinematics cache and body poses, the dof-block tables, and the wave primitives (DPP sums,
// maxima, scans).  Relies only on mmx_step.inc's own macros and constants (WG, LANE, SYNC, NSLOT, LD, ...) and
// the headers it includes.
// ============================================================================ per-env LDS
// LDS contact record: distance, position, normal and one int (bits): the 15-bit order key (pair x 8 +
// local order, the sort key) | geom 1 << 16 | geom 2 << 22 (the bodies are the geoms' bodies)
enum { CL_DIST = 0, CL_POS = 1, CL_N = 4, CL_KEY = 7, CL_F };
static_assert(MMX_NGEOM <= 64 && MMX_NPAIR * 8 < 65536, "contact key packing");
// contact c's record in the field-major array E.con[field][contact] (a lane reading its own contact
// reads consecutive words: no LDS bank conflicts at the 8-float record size)
struct CRec {
  const float* b;
  int c;
  DEV float operator[](int k) const { return b[k * MMX_MAXCON + c]; }
};
struct CRecW {
  float* b;
  int c;
  DEV float& operator[](int k) const { return b[k * MMX_MAXCON + c]; }
};
// a contact record held in registers (the row build: lane c holds contact c)
struct CReg {
  float v[CL_F];
  DEV float operator[](int k) const { return v[k]; }
};
template <class R>
DEV int con_key(const R& c) { return __float_as_int(c[CL_KEY]); }
template <class R>
DEV int con_g1(const R& c) { return (con_key(c) >> 16) & 63; }
template <class R>
DEV int con_g2(const R& c) { return (con_key(c) >> 22) & 63; }
// Hessian staging tile row stride: 17, so the dof lanes' reads of different tile rows (tile_gather)
// fall on different banks (a 16-float stride put rows sd and sd + 2 on one bank: up to 5-way; with the
// polygon stride below, LDS bank conflicts 0.31 -> 0.12 per LDS-active cycle, +0.2 % in the A/B)
#define GST 17
struct EnvSh {
  float qpos[30], qvel[28], ctrl[8];
  float target[4];
  float bx[NSLOT][3], bR[NSLOT][9];
  float S[9][6];
  // mass matrix: the arm's 9 x 9 block (the 3 free cubes are separate trees whose 6 x 6 blocks are
  // diagonal: mass x3, principal inertia x3, centre of mass at the joint)
  float M9[9][9];
  // x: the Newton solution; between solves it holds the warm start for the next one (MuJoCo's
  // qacc_warmstart: the record's qacc_ws is loaded into it and stored from it)
  float qfrc[LD], qacc_s[LD], x[LD], p[LD];
  // constraint rows in block format: a row touches at most two dof blocks (arm = 9 dofs,
  // cube k = 6 dofs); J[i][0..n0) holds block b0's columns, J[i][n0..n0+n1) block b1's;
  // J doubles as the contact-sort scratch in collide_wave (rows are built after it).
  // Rows come in aligned groups of 4: the equality / joint-limit rows (padded to a multiple of 4),
  // then per contact its 4 BASIS rows (normal, tangent 1, tangent 2, torsion; rows the contact's
  // condim does not use are zero rows).  MuJoCo's pyramid edges J_n +/- mu_k J_k are never
  // stored: the solver forms them from the basis rows (2/3 of the storage and MFMA steps).
  // Rows past MMX_LDSEFC (a pile of contacts) live in the env's HBM overflow block `ovf` (J rows,
  // then D, then NC): lane-owned row q >= LDSEFC / 64 is always an HBM row.
  // Chunk-major (r04): chunk q (slots 4q..4q+3) of row i at J[q][i], a chunk-row stride of
  // MMX_LDSEFC + 1 chunks.  A row-per-lane read of chunk q is one ds_read_b128 at an immediate
  // offset with consecutive lanes on consecutive 16-byte bank quads (conflict-free); the Hessian
  // staging's reads of one row's slot (lane & 15) land on 16 different banks.  Row-major 64-byte
  // rows put lanes 4 apart on one bank (4-way): LDS bank conflicts 0.71 -> 0.31 cycles per
  // LDS-active cycle, +0.75 % env steps/s at unchanged VALU (A/B, DESIGN §2).
  alignas(16) float J[4][MMX_LDSEFC + 1][4];  // J[k >> 2][i][k & 3] = slot k of row i (past the width 0; 15 = aref)
  unsigned char hdr[MMX_LDSEFC];  // b0 | b1 << 4 (block 15 = none); row 0 is the equality (rows past: ovf)
  // D: the row's 1 / R while the rows are built (doubling as the row -> contact map before) and in
  // the solver's setup; then per Newton iteration the diagonal entry of the group's edge-weight
  // matrix C (C_kk; a single row's active weight).  NC: C_nk, the row's coupling to its contact's
  // normal row (0 for single and normal rows).
  alignas(16) float D[MMX_LDSEFC];
  alignas(16) float NC[MMX_LDSEFC];
  // the Newton Hessian's 16 x 16 staging tile (row stride GST); the collision scratch before the rows
  alignas(16) float G[16 * GST];
  float* ovf;  // this env's overflow block (S.efc_ovf + i * MMX_OVF_F): rows past LDSEFC, headers, list
  int ncon, nefc, flags;
  int nsingle;  // rows [0, nsingle): equality + limit rows (+ zero padding); contact groups after
  int nefc_mj;  // MuJoCo's row count (pyramid edges + equality + limits), for the statistics
  int ncls[3];    // collision candidates per narrowphase class (plane, box-box, GJK)
  int tbase[11];  // rows are grouped by block-pair type: type t owns rows [tbase[t], tbase[t+1])
  int act_free;  // bit a: actuator a's force is inside its forcerange (its kv enters qDeriv)
  float stats[STAT_N];  // lane 0 accumulates; loaded / stored with the env record
  // persistent broadphase list (collide_prune; its entries in the overflow block, cand_of): the pairs
  // within MMX_CAND_MARGIN of contact when it was built, in pair order; valid while the bodies'
  // accumulated displacement bound stays under half the margin.  ncand < 0: no valid list (every
  // record load invalidates it).
  float cdisp;     // bound on any geom's displacement since the build (x 2: a pair's relative one)
  float crad;      // max over moving geoms of |geom centre - body origin| + bounding radius
  float cspd;      // one-wave build: this substep's max arm-body speed (origin + angular x crad; from the RNE)
  int ncand;
};
// The workgroup's env lives in one file-scope LDS object: the non-inlined substep function below
// reaches it by symbol (LDS address space), not through a generic pointer.
static __shared__ EnvSh g_E;
// twelve workgroups (envs) per CU share its 160 KiB of LDS, allocated in 1,280-byte blocks (measured:
// tools/calib/lds_occ.hip, profiles/r05_lds_residency.json): the occupancy the kernel is tuned for (r06;
// r05: eleven; with 192 LDS rows, MMX_LDSEFC=192, four, each with a helper wave).  Twelve waves are three per SIMD, the
// 168-VGPR budget of amdgpu_waves_per_eu(3).
static_assert(MMX_LDSEFC != 128 || (sizeof(EnvSh) + 1279) / 1280 * 1280 * 12 <= 160 * 1024,
              "EnvSh no longer fits 12 envs per CU");
static_assert((sizeof(EnvSh) + 1279) / 1280 * 1280 * 8 <= 160 * 1024, "EnvSh no longer fits 8 envs per CU");

// The scratch region: E.J, E.hdr, E.D, E.NC and E.G (contiguous in EnvSh) hold the phases' scratch
// outside the constraint build + Newton solve (rows are rebuilt every substep): the collision layout
// below (geom records, candidates, the contacts, the narrowphase work space), the position stage's chain
// scan, the IK system, the RNE / composite-inertia / actuator scratch of the dynamics (at COL_WORK) and
// the observation of the step end.  The contacts live here from the narrowphase to the row build, whose
// lanes take them into registers (lane c: contact c) before the first row is written; the Newton
// Hessian staging tile is E.G.
// r06: the contacts out of their own LDS array (into this region, then registers), the rows' mu passed
// to the solver in registers, the overflow rows' headers and the broadphase list in the HBM overflow
// block: 12,640 B of LDS, twelve envs per CU (r05: 14,080 B with its own contact array, eleven; r04:
// 20,432 B with 192 rows, eight); rows past 128 go to the HBM overflow block.
#define GXS 17        // geom record: world pose (x 3, R 9), rbound, type, box half extents (3)
#define GX_RB 12
#define GX_TYPE 13
#define GX_HALF 14
#define COL_GX 0      // [NGEOM][GXS]
#define COL_CAND ((MMX_NGEOM * GXS + 15) & ~15)  // [COL_LIST] candidate pairs after the sphere test, then by class
#ifndef MMX_COL_LIST
#define MMX_COL_LIST 320  // more survivors of the sphere test than this: the rest are dropped, SHF_CON_OVF
#endif
#define COL_LIST MMX_COL_LIST
#define COL_CON (COL_CAND + COL_LIST)   // the contacts, field-major [CL_F][MMX_MAXCON] (crec)
#define COL_WORK (COL_CON + CL_F * MMX_MAXCON)  // narrowphase work space: box-box polygons, the EPA polytope
#define COL_POLY 49                     // (GJK pass), then the contact sort (49: the quads' polygons
                                        // start on different banks; 48 put quads 2 apart on one)
#define COL_PLANES 16                   // box-box lane quads per pass: one polygon each
#define COL_EPA COL_WORK
static_assert(offsetof(EnvSh, hdr) == offsetof(EnvSh, J) + sizeof(EnvSh::J) &&
                  offsetof(EnvSh, D) == offsetof(EnvSh, hdr) + sizeof(EnvSh::hdr) &&
                  offsetof(EnvSh, NC) == offsetof(EnvSh, D) + sizeof(EnvSh::D) &&
                  offsetof(EnvSh, G) == offsetof(EnvSh, NC) + sizeof(EnvSh::NC),
              "the scratch region must be contiguous");
#define SCR_FLOATS ((int)((offsetof(EnvSh, G) + sizeof(EnvSh::G) - offsetof(EnvSh, J)) / 4))
static_assert(COL_EPA + EPA_SCRATCH_FLOATS <= SCR_FLOATS, "EPA scratch exceeds the scratch region");
static_assert(COL_WORK + MMX_MAXCON * CL_F <= SCR_FLOATS, "contact sort exceeds the scratch region");
static_assert(COL_CON % 4 == 0 && COL_WORK % 4 == 0, "16-byte aligned collision scratch blocks");
static_assert(COL_WORK + COL_PLANES * COL_POLY <= SCR_FLOATS, "box-box polygons exceed the scratch region");
static_assert(MMX_CAND_CAP <= COL_LIST && MMX_NPAIR < 4096, "collision scratch layout");

// The 192-row build (one env per CU quarter, C2's batches) gives each env a second wave, the
// "helper": per substep it runs the IK beside the env wave's kinematics, then the dynamics (RNE, CRBA,
// smooth forces) beside the broadphase, then the GJK / EPA pairs beside the plane and box-box pairs
// (mj_step_wave).  Its scratch (IK system, dynamics, EPA polytope, one after the other) sits past
// everything the env wave's collision uses (the 192-row scratch region has the room); the 128-row build
// runs the phases in turn on one wave and keeps them in the narrowphase work space.
#ifndef MMX_STEP_HELPER
#define MMX_STEP_HELPER (MMX_LDSEFC == 192)
#endif
#if MMX_STEP_HELPER
#define COL_END (COL_WORK + EPA_SCRATCH_FLOATS)  // the collision's scratch ends here (asserted below)
static_assert(COL_WORK + COL_PLANES * COL_POLY <= COL_END && COL_WORK + MMX_MAXCON * CL_F <= COL_END,
              "the narrowphase work space exceeds COL_END");
#define SCR_DYN ((COL_END + 3) & ~3)
#define SCR_IKW SCR_DYN  // the IK system [72] (before the dynamics, on the helper)
#define SCR_EPA SCR_DYN  // the helper's EPA polytope (after the dynamics)
#else
#define SCR_DYN COL_WORK
#define SCR_IKW 0
#define SCR_EPA COL_EPA
#endif
// SCR_DYN: RNE frc + inertia [12][16], subtree force [12][6] (264), then:
#define SCR_IC (SCR_DYN + 272)     // composite inertias [12][10]
#define SCR_AF (SCR_IC + 120)      // actuator forces [8]
#define SCR_BIAS (SCR_AF + 8)      // RNE bias force of the arm dofs [9]
#define SCR_OBS COL_WORK           // observation (step end after its contact scan, reset, forward)
#define SCR_ACT (COL_WORK + 96)    // raw action of the step (lane 0, before the substeps)
static_assert(SCR_BIAS + 9 <= SCR_FLOATS && SCR_OBS + MMX_NOBS <= SCR_ACT && SCR_ACT + 12 <= SCR_FLOATS &&
                  SCR_EPA + EPA_SCRATCH_FLOATS <= SCR_FLOATS && SCR_IKW + 72 <= SCR_FLOATS,
              "scratch layout");
// Test builds only (libmmx_hdelay.so / libmmx_edelay.so, tests/test_helper_layout.py): one of the
// env's two waves is held back right after barriers C and A of every substep (1: the helper wave,
// before its IK and before its dynamics; 2: the env wave, before its kinematics and before its prune), so
// whatever one wave reads from LDS while the other writes it shows as a difference between the two
// builds.  The hold must outlast the longest phase the other wave runs meanwhile: the dynamics, 11.6 k
// cycles per substep (kinematics 6.0 k, IK 4.2 k: profiles/r06_fsm_profile.json), and twice that for
// margin is 23 k.  s_sleep waits 64 clocks per unit of its 7-bit operand, so 127 is ~8.1 k clocks and
// MMX_DELAY_SLEEPS = 4 of them ~32.5 k (~1 M cycles per env step: 16 substeps x 2 holds).  The product
// build (0) contains none of it.
#ifndef MMX_HELPER_DELAY
#define MMX_HELPER_DELAY 0
#endif
#if MMX_HELPER_DELAY && MMX_STEP_HELPER
#define MMX_DELAY_SLEEPS 4
DEV void delay_wave() {
#pragma unroll
  for (int k = 0; k < MMX_DELAY_SLEEPS; k++) __builtin_amdgcn_s_sleep(127);
  asm volatile("" ::: "memory");  // no LDS access of the phase that follows is moved above the hold
}
#define DELAY_HELPER() do { if (MMX_HELPER_DELAY == 1) delay_wave(); } while (0)
#define DELAY_ENV() do { if (MMX_HELPER_DELAY == 2) delay_wave(); } while (0)
#else
#define DELAY_HELPER() do { } while (0)
#define DELAY_ENV() do { } while (0)
#endif
DEV float* scr_of(EnvSh& E) { return reinterpret_cast<float*>(&E.J); }
DEV const float* scr_of(const EnvSh& E) { return reinterpret_cast<const float*>(&E.J); }
DEV float* obs_of(EnvSh& E) { return scr_of(E) + SCR_OBS; }
DEV const float* obs_of(const EnvSh& E) { return scr_of(E) + SCR_OBS; }
// the contacts (from the narrowphase to the row build, which takes them into registers)
DEV float* con_of(EnvSh& E) { return scr_of(E) + COL_CON; }
DEV CRec crec(const EnvSh& E, int c) { return CRec{scr_of(E) + COL_CON, c}; }
DEV float* lrow_of(EnvSh& E) { return E.G; }  // the Hessian staging tile
// the general (cube-cube coupled) Cholesky's 27 x 27 transpose: rare, so in the env's HBM overflow
// block after the overflow rows, not in LDS
DEV float* arrow_of(EnvSh& E) { return E.ovf + MMX_OVF_ARROW_AT(MMX_LDSEFC); }
// the persistent broadphase list (16-bit pair indices) in the overflow block
DEV unsigned short* cand_of(const EnvSh& E) { return reinterpret_cast<unsigned short*>(E.ovf + MMX_OVF_CAND_AT(MMX_LDSEFC)); }
// the GJK pair class's table of separating axes in the overflow block (mmx_gjk_cache.h; AxisCache in mmx_geom.h)
DEV float* axis_of(const EnvSh& E) { return E.ovf + MMX_OVF_AXIS_AT(MMX_LDSEFC); }
// Constraint row i: J in E.J[.][i] (chunk-major) and D in E.D[i] for i < MMX_LDSEFC, else in the env's HBM
// overflow block (J rows [OVFEFC][16], then D [OVFEFC]).  For a lane-owned row i = LANE + 64 q the
// test folds at compile time (LANE's known bits), so the unrolled loops carry no branch.
static_assert(MMX_LDSEFC % WG == 0 && MMX_LDSEFC <= MMX_MAXEFC, "LDS rows: whole lane slices");
DEV float* ovf_j(const EnvSh& E, int i) { return E.ovf + 16 * (i - MMX_LDSEFC); }
DEV float* ovf_d(const EnvSh& E, int i) { return E.ovf + 16 * MMX_OVFEFC + (i - MMX_LDSEFC); }
DEV float* ovf_nc(const EnvSh& E, int i) { return E.ovf + 17 * MMX_OVFEFC + (i - MMX_LDSEFC); }
DEV float& jlds(EnvSh& E, int i, int k) { return E.J[k >> 2][i][k & 3]; }
DEV const float& jlds(const EnvSh& E, int i, int k) { return E.J[k >> 2][i][k & 3]; }
DEV float4 jrow4(const EnvSh& E, int i, int q) {
  if (i >= MMX_LDSEFC) return reinterpret_cast<const float4*>(ovf_j(E, i))[q];
  return *reinterpret_cast<const float4*>(E.J[q][i]);
}
DEV float jget(const EnvSh& E, int i, int k) { return i < MMX_LDSEFC ? jlds(E, i, k) : ovf_j(E, i)[k]; }
DEV void jset(EnvSh& E, int i, int k, float v) {
  if (i < MMX_LDSEFC) jlds(E, i, k) = v;
  else ovf_j(E, i)[k] = v;
}
DEV float dget(const EnvSh& E, int i) { return i < MMX_LDSEFC ? E.D[i] : *ovf_d(E, i); }
DEV void dset(EnvSh& E, int i, float v) {
  if (i < MMX_LDSEFC) E.D[i] = v;
  else *ovf_d(E, i) = v;
}
DEV float ncget(const EnvSh& E, int i) { return i < MMX_LDSEFC ? E.NC[i] : *ovf_nc(E, i); }
// row headers: LDS for the LDS rows, the overflow block's byte array for the rest
DEV unsigned char* ovf_hdr(const EnvSh& E) { return reinterpret_cast<unsigned char*>(E.ovf + MMX_OVF_HDR_AT(MMX_LDSEFC)); }
DEV int hdr_get(const EnvSh& E, int i) { return i < MMX_LDSEFC ? E.hdr[i] : ovf_hdr(E)[i - MMX_LDSEFC]; }
DEV void hdr_set(EnvSh& E, int i, int h) {
  if (i < MMX_LDSEFC) E.hdr[i] = (unsigned char)h;
  else ovf_hdr(E)[i - MMX_LDSEFC] = (unsigned char)h;
}
DEV void ncset(EnvSh& E, int i, float v) {
  if (i < MMX_LDSEFC) E.NC[i] = v;
  else *ovf_nc(E, i) = v;
}
// rows written by one lane and read by another: HBM rows need the wave's stores complete first
// (workgroup scope = s_waitcnt vmcnt(0); the CU's L1 is shared by the wave).  Uniform branch.
DEV void ovf_fence(int nefc) {
  if (nefc > MMX_LDSEFC) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}
// the last substep's contacts (diagnostic copy, mmx_buffers.contacts), stored before the row build
// overwrites the scratch region that holds them
DEV void store_contacts(float* dst, const EnvSh& E) {
  const int n = E.ncon;
  for (int c = LANE; c < MMX_MAXCON; c += WG) {  // the 13-field record (CON_*) of LDS contact c
    float* o = dst + (size_t)c * CON_F;
    const CRec l = crec(E, c);
    const int g1 = c < n ? con_g1(l) : 0, g2 = c < n ? con_g2(l) : 0;
    o[CON_DIST] = c < n ? l[CL_DIST] : 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      o[CON_POS + k] = c < n ? l[CL_POS + k] : 0.f;
      o[CON_N + k] = c < n ? l[CL_N + k] : 0.f;
      o[CON_MU0 + k] = c < n ? fmaxf(MMX_geom_friction[3 * g1 + k], MMX_geom_friction[3 * g2 + k]) : 0.f;
    }
    o[CON_DIM] = c < n ? (float)max(MMX_geom_condim[g1], MMX_geom_condim[g2]) : 0.f;
    o[CON_G1] = c < n ? (float)g1 : 0.f;
    o[CON_G2] = c < n ? (float)g2 : 0.f;
  }
}
DEV float* contacts_dst(const MMXState& S, int i) { return S.con + (size_t)i * MMX_MAXCON * CON_F; }
enum { SHF_ROBOT_OBST = 1, SHF_CON_OVF = 2, SHF_EFC_OVF = 4, SHF_NAN = 8 };

DEV int body_slot(int b) { return b <= 11 ? b - 1 : b - 5; }
// The IK's kinematics cache (KIN_*: hand pose, arm joint axes and anchors, cube positions of the
// last position stage, the HBM record's kin[]) is not a separate LDS array: its entries ARE the
// position stage's outputs (hand slot of bx / bR, angular part of S, joint and cube bodies' bx), which stay
// untouched from one position stage to the next IK.  load_env scatters the record into them,
// store_env gathers it back.
DEV float& kin_ref(EnvSh& E, int k) {
  if (k < KIN_HAND_MAT) return E.bx[body_slot(MMX_BODY_HAND)][k - KIN_HAND_POS];
  if (k < KIN_AXIS) return E.bR[body_slot(MMX_BODY_HAND)][k - KIN_HAND_MAT];
  if (k < KIN_ANCHOR) return E.S[(k - KIN_AXIS) / 3][(k - KIN_AXIS) % 3];
  if (k < KIN_OBJ) return E.bx[body_slot(MMX_jnt_body[(k - KIN_ANCHOR) / 3])][(k - KIN_ANCHOR) % 3];
  return E.bx[11 + (k - KIN_OBJ) / 3][(k - KIN_OBJ) % 3];
}
DEV float kin_get(const EnvSh& E, int k) { return kin_ref(const_cast<EnvSh&>(E), k); }
DEV int body_block(int b) { return (b >= 2 && b <= 11) ? 0 : (b >= 16 ? b - 15 : -1); }
#define BLK_NONE 15
DEV int blk_size(int b) { return b == 0 ? 9 : (b == BLK_NONE ? 0 : 6); }
DEV int blk_d0(int b) { return b == 0 ? 0 : 9 + 6 * (b - 1); }
DEV int dof_blk(int a) { return a < 9 ? 0 : 1 + (a - 9) / 6; }
// slot of dof a in a row with header h, or -1 if the row does not touch a
DEV int row_slot(int h, int a) {
  const int b0 = h & 15, b1 = (h >> 4) & 15, ba = dof_blk(a);
  if (ba == b0) return a - blk_d0(b0);
  if (ba == b1) return blk_size(b0) + a - blk_d0(b1);
  return -1;
}
// block-pair row types: (0,-) (0,1) (0,2) (0,3) (1,-) (1,2) (1,3) (2,-) (2,3) (3,-)
#define NTYPE 10
static constexpr int kTB0[NTYPE] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 3};
static constexpr int kTB1[NTYPE] = {15, 1, 2, 3, 15, 2, 3, 15, 3, 15};
DEV int row_type(int b0, int b1) {
  return b0 == 0 ? (b1 == BLK_NONE ? 0 : b1) : (b0 == 1 ? (b1 == BLK_NONE ? 4 : 3 + b1) : (b0 == 2 ? (b1 == BLK_NONE ? 7 : 8) : 9));
}
DEV bool arm_anc(int d, int b) { return d <= 6 ? (b >= d + 2 && b <= 11) : (d == 7 ? b == 10 : b == 11); }
// the arm dofs on body b's root path as a 9-bit mask (bit d = arm_anc(d, b)): the chain dofs
// 0..min(b - 2, 6), plus finger dof 7 / 8 for the finger bodies 10 / 11
DEV unsigned anc_mask(int b) {
  return b >= 2 && b <= 11 ? ((1u << min(b - 1, 7)) - 1u) | (b == 10 ? 0x80u : 0u) | (b == 11 ? 0x100u : 0u) : 0u;
}
DEV V3 body_x(const EnvSh& E, int b) {
  if (MMX_body_static[b]) return V3{0.f, 0.f, 0.f};
  const int s = body_slot(b);
  return V3{E.bx[s][0], E.bx[s][1], E.bx[s][2]};
}
DEV M3 body_R(const EnvSh& E, int b) {
  M3 R;
  const int s = body_slot(b);
#pragma unroll
  for (int k = 0; k < 9; k++) R.m[k] = E.bR[s][k];
  return R;
}
DEV SV load_S(const EnvSh& E, int d) { return SV{V3{E.S[d][0], E.S[d][1], E.S[d][2]}, V3{E.S[d][3], E.S[d][4], E.S[d][5]}}; }

// ---------------------------------------------------------------- wave primitives
// wave64 sum: DPP butterflies inside each row of 16 lanes, then the four row sums in a fixed
// order (bit-identical in every lane, no LDS traffic)
// (update_dpp with old = 0 and bound_ctrl: every control used here reads a valid lane, so the value
// is the same as mov_dpp's, but LLVM's DPP combiner only folds this form into the consuming VOP2
// op: v_add_f32_dpp instead of v_mov_b32_dpp + v_add_f32)
template <int CTRL>
DEV float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
DEV float wave_sum(float v) {
  v += dpp_f<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_f<0x141>(v);  // row_half_mirror
  v += dpp_f<0x140>(v);  // row_mirror
  return (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)) +
          __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16))) +
         (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)) +
          __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48)));
}
DEV float readlane_max0(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)); }
DEV float wave_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  v = fmaxf(v, dpp_f<0x140>(v));
  return fmaxf(fmaxf(readlane_max0(v), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16))),
               fmaxf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)),
                     __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48))));
}
// wave64 inclusive prefix sum: DPP row_shr butterflies inside each row of 16 lanes, then the
// row totals (v_readlane) are added to the rows above
DEV int wave_scan_incl(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);  // row_shr:8
  const int r0 = __builtin_amdgcn_readlane(v, 15), r1 = __builtin_amdgcn_readlane(v, 31);
  const int r2 = __builtin_amdgcn_readlane(v, 47);
  const int row = LANE >> 4;
  return v + (row == 0 ? 0 : (row == 1 ? r0 : (row == 2 ? r0 + r1 : r0 + r1 + r2)));
}
// triangular index e -> (a, b) with a >= b, e = a(a+1)/2 + b
DEV void tri_index(int e, int& a, int& b) {
  int aa = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
  while ((aa + 1) * (aa + 2) / 2 <= e) aa++;
  while (aa * (aa + 1) / 2 > e) aa--;
  a = aa;
  b = e - aa * (aa + 1) / 2;
}
