// Part 5 of mmx_step.inc (an ordered fragment, included there and nowhere else): the Newton solver,
// newton_wave and what it is made of (the cost and line search, the MFMA Hessian / gradient pass and its
// delta pass, the block Cholesky solves), and RPL, the rows a lane owns, which the parts after it use too.
// Relies on the row accessors (jget / dget / hdr_get ...), the block tables and the wave primitives of the lds
// part, row_bcast of the dynamics part and the rows make_constraints_wave (constraints) left in LDS.
// In this file, from the next line to the restore in its last, LANE is the opaque lane id (lane_opaque in
// mmx_step.inc says why here and nowhere else).
#undef LANE
#define LANE lane_opaque()
// ============================================================================ Newton solver (wave)
// Primal Newton with exact line search (MuJoCo's default solver): minimise
//   0.5 (x - xs)' M (x - xs) + sum_i s_i(J_i x - aref_i),  s_i = 0.5 D_i r^2 on active rows.
// Lane l owns constraint rows l + 64 q (q < RPL): their residual, search-direction projection,
// D and equality flag stay in registers through the line search.  The Hessian and gradient come
// from one MFMA pass (hess_grad_mfma) straight into registers; the Cholesky factorisation and
// both triangular solves run in registers (chol_solve).
#define RPL ((MMX_MAXEFC + WG - 1) / WG)

DEV float readlane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// Newton lane layout: the solver's dof-space values (Hessian rows, gradient, search direction,
// M v) sit with arm dof d in lane d (DPP row 0 of the wave's four 16-lane rows) and cube b's dof k
// in lane 16 b + k (row b), so each dof block owns one DPP row: the block Cholesky broadcasts a
// pivot to its block with one row_newbcast.  Lanes 9..15, 16 b + 6..15 hold no dof (-1).
DEV int newton_dof(int L) {
  const int r = L >> 4, k = L & 15;
  return r == 0 ? (k < 9 ? k : -1) : (k < 6 ? 9 + 6 * (r - 1) + k : -1);
}
__host__ __device__ constexpr int newton_lane(int d) { return d < 9 ? d : 16 * (1 + (d - 9) / 6) + (d - 9) % 6; }

// J_i . x for a block-format row (slots past the row's width hold zeros)
DEV float row_dot16(const EnvSh& E, int i, const float* x) {
  const int h = hdr_get(E, i), b0 = h & 15, b1 = (h >> 4) & 15;
  const int n0 = blk_size(b0), o0 = blk_d0(b0), o1 = (b1 == BLK_NONE ? 0 : blk_d0(b1)) - n0;
  float jv[16];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const float4 v = jrow4(E, i, q);
    jv[4 * q] = v.x;
    jv[4 * q + 1] = v.y;
    jv[4 * q + 2] = v.z;
    jv[4 * q + 3] = v.w;
  }
  // slot k holds dof k + o0 below n0 and dof k + o1 from n0 on (n0 = 9 for an arm block, 6 for a
  // cube), so slots 0..5 read from one base, 6..8 from the base n0 selects, 9..11 from the second
  // one: LDS reads with immediate offsets instead of a per-slot index select.  Slots 12..14 are
  // clamped to dof 26 (past the row's width they hold zeros; the clamp keeps the read in x).
  const float* x0 = x + o0;
  const float* x1 = x + o1;
  const float* x2 = n0 == 9 ? x0 : x1;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 15; k++) {
    const float v = k < 6 ? x0[k] : (k < 9 ? x2[k] : (k < 12 ? x1[k] : x[min(o1 + k, 26)]));
    s = fmaf(jv[k], v, s);
  }
  return s;
}

// the cubes' diagonal mass matrix entry of free dof k (0..17: cube k / 6, mass x3 then principal
// inertia x3): model constants, not per env
DEV float mass_cube(int k) {
  const int b = 16 + k / 6, rr = k % 6;
  return rr < 3 ? MMX_body_mass[b] : MMX_body_inertia[9 * b + 4 * (rr - 3)];
}
// (M v) of the lane's dof (Newton lane layout; arm rows: the 9 x 9 block; cube rows: the diagonal)
DEV float mass_mul(const EnvSh& E, const float* v) {
  const int nd = newton_dof(LANE);
  if (LANE < 9) {
    float m = 0.f;
#pragma unroll
    for (int b = 0; b < 9; b++) m = fmaf(E.M9[LANE][b], v[b], m);
    return m;
  }
  return nd >= 0 ? mass_cube(nd - 9) * v[nd] : 0.f;
}
// (M (xa - xb)) of the lane's dof, same layout
DEV float mass_mul_diff(const EnvSh& E, const float* xa, const float* xb) {
  const int nd = newton_dof(LANE);
  if (LANE < 9) {
    float m = 0.f;
#pragma unroll
    for (int b = 0; b < 9; b++) m = fmaf(E.M9[LANE][b], xa[b] - xb[b], m);
    return m;
  }
  return nd >= 0 ? mass_cube(nd - 9) * (xa[nd] - xb[nd]) : 0.f;
}

// Pyramid edges from basis rows.  Lane l owns rows l + 64 q; rows are 4-aligned groups, so a
// group's rows sit in one DPP quad (lanes 4m..4m+3).  A row's role: single (equality / limit /
// padding row: one edge, itself), normal row of a contact (no edge of its own), basis row k >= 1 of
// a contact (the two edges J_n +/- mu_k J_k; mu < 0: unused row, no edge).  Edge e of the lane's
// row is a_e (normal row value) + b_e (own value), for residuals and for J p alike.
struct EdgeCoef {
  float a0, b0, a1, b1;  // edge 0: a0 n + b0 own, edge 1: a1 n + b1 own; all 0 for a missing edge
};
// (no boolean per edge: a missing edge has zero coefficients, so its value is 0 and never
// active; only the finger equality, row 0 = lane 0 of slice 0, is active at any sign)
DEV EdgeCoef edge_coef(int i, int nefc, int nsingle, float mu) {
  EdgeCoef c;
  const bool valid = i < nefc;
  const bool single = valid && i < nsingle;
  const bool krow = valid && !single && (i & 3) != 0 && mu >= 0.f;
  c.a0 = krow ? 1.f : 0.f;
  c.b0 = krow ? mu : (single ? 1.f : 0.f);
  c.a1 = c.a0;
  c.b1 = krow ? -mu : 0.f;
  return c;
}
// the finger equality row (always active): row 0, owned by lane 0 in slice 0
#define EQROW(q) ((q) == 0 && LANE == 0)
// value held by the first lane of the caller's DPP quad (the group's normal row)
DEV float quad_first(float v) { return dpp_f<0x00>(v); }  // quad_perm [0,0,0,0]
DEV float quad_sum(float v) {
  v += dpp_f<0xB1>(v);  // quad_perm [1,0,3,2]
  return v + dpp_f<0x4E>(v);  // quad_perm [2,3,0,1]
}

// cost at two candidate points (warm start, qacc_smooth) in one pass; also returns, per lane,
// the basis-row residuals J x - aref of the rows it owns and (M (x - xs))_lane for both
// candidates, so the Newton loop starts from them and then only updates them (r += a J p,
// M dx += a M p).  Edge cost 0.5 D e^2 on active edges (e < 0, or the equality).
DEV void cost2_wave(const EnvSh& E, const float* xa, const float* xb, const float* mu, const float* dd, float& ca,
                    float& cb, float* va, float* vb, float& ma, float& mb) {
  float c0 = 0.f, c1 = 0.f;
  ma = 0.f;
  mb = 0.f;
  const int nd = newton_dof(LANE);
  if (nd >= 0) {
    ma = mass_mul_diff(E, xa, E.qacc_s);
    mb = mass_mul_diff(E, xb, E.qacc_s);
    c0 = 0.5f * (xa[nd] - E.qacc_s[nd]) * ma;
    c1 = 0.5f * (xb[nd] - E.qacc_s[nd]) * mb;
  }
  const int nefc = E.nefc, nsingle = E.nsingle;
#pragma unroll
  for (int q = 0; q < RPL; q++) {
    const int i = LANE + WG * q;
    va[q] = 0.f;
    vb[q] = 0.f;
    if (WG * q >= nefc) continue;  // uniform: the slice holds no row
    if (i < nefc) {
      const float aref = jget(E, i, 15);
      va[q] = row_dot16(E, i, xa) - aref;
      vb[q] = row_dot16(E, i, xb) - aref;
    }
    const float na = quad_first(va[q]), nb = quad_first(vb[q]);
    const EdgeCoef ec = edge_coef(i, nefc, nsingle, mu[q]);
    const float ea0 = fmaf(ec.a0, na, ec.b0 * va[q]), ea1 = fmaf(ec.a1, na, ec.b1 * va[q]);
    const float eb0 = fmaf(ec.a0, nb, ec.b0 * vb[q]), eb1 = fmaf(ec.a1, nb, ec.b1 * vb[q]);
    const float h = 0.5f * dd[q];
    c0 += (EQROW(q) || ea0 < 0.f ? h * ea0 * ea0 : 0.f) + (ea1 < 0.f ? h * ea1 * ea1 : 0.f);
    c1 += (EQROW(q) || eb0 < 0.f ? h * eb0 * eb0 : 0.f) + (eb1 < 0.f ? h * eb1 * eb1 : 0.f);
  }
  ca = wave_sum(c0);
  cb = wave_sum(c1);
}

// J'WJ and J'W r on the matrix cores, one block-pair row type at a time.  Rows of a type share
// their slot -> dof map, so in slot space the type's contribution is a 16 x 16 tile.  Over the
// pyramid edges J_e = c_e' B of a 4-row group B (c_e = e_n +/- mu_k e_k), sum_e w_e J_e' J_e =
// B' C B with the group's 4 x 4 edge-weight matrix C = sum_e w_e c_e c_e' (an arrow: C_nn, C_nk,
// C_kk), and sum_e w_e r_e J_e' = B' g.  So G = sum_groups B' [C B | g]:
// v_mfma_f32_16x16x4_f32 with A[slot i][row k] = B[k][i] and B-operand[row k][slot j] =
// (C B)[k][j] = C_kk B[k][j] + (k == n ? sum_m C_nm B[m][j] : C_nk B[n][j]), where slot 15
// (always 0 in J) carries g_k instead, so G[:, 15] is the type's gradient.  Single rows form
// groups with a diagonal C (their active weights).  Lane l supplies row (l >> 4) of the step's
// group at slot l & 15: contiguous reads of the block-format rows.  Each tile is staged in LDS and gathered by the
// dof lanes into their Hessian row (static columns) and gradient.  Returns, in lane j < 27,
// row j of H = M + J'WJ in hrow[0..27) and g_j = (M (x - xs) + J'W r)_j.
typedef float f32x4 __attribute__((ext_vector_type(4)));
// groups (MFMA steps) per trip, their loads issued together (3 or 4: -1.3 / -0.7 % in the r03 A/B)
#define MMX_HESS_U 2
// gather one row type's staged 16 x 16 tile into the dof lanes' Hessian rows: dof lane d reads row
// sd of the tile; the type's two blocks land on static columns of hrow (uniform branches over the
// 4 possible blocks keep every register index static); slot 15 is the type's gradient
DEV void tile_gather(const float* G, int t, int bd, int od, float* hrow, float& gacc) {
  const int b0 = kTB0[t], b1 = kTB1[t];
  const int n0 = blk_size(b0);
  const int sd = bd == b0 ? od : (bd == b1 ? n0 + od : -1);
  if (sd >= 0) {
    const float* Gr = G + GST * sd;
#pragma unroll
    for (int B = 0; B < 4; B++) {
      const int nb = B == 0 ? 9 : 6, dB = B == 0 ? 0 : 9 + 6 * (B - 1);
      if (B == b0) {
#pragma unroll
        for (int k = 0; k < nb; k++) hrow[dB + k] += Gr[k];
      } else if (B == b1) {
#pragma unroll
        for (int k = 0; k < nb; k++) hrow[dB + k] += Gr[n0 + k];
      }
    }
    gacc += Gr[15];
  }
}
// row types staged per barrier round.  3 measured -1.3 % in the r03 A/B, when E.con held three
// 16 x 16 tiles and the unrolled rounds grew the register save area the substep then had; since the
// LDS shrink E.con (MMX_MAXCON * CL_F = 512 floats) holds one tile of 16 * GST = 272, so only 1 builds
#define HESS_TILES 1
static_assert(HESS_TILES * 16 * GST <= MMX_MAXCON * CL_F, "Hessian staging tiles exceed E.con");
DEV float hess_grad_mfma(EnvSh& E, int nefc, float* hrow, float mdx) {
  float* stats = E.stats;
  CLK_DECL;
  float* G = lrow_of(E);  // 16 x 16 staging tile (the factor's space is free until the Cholesky)
  const int col = LANE & 15, rk = LANE >> 4;
  // the lane's dof (Newton lane layout): block LANE >> 4, offset LANE & 15 in it
  const int nd = newton_dof(LANE), d = max(nd, 0);
  const int bd = nd >= 0 ? LANE >> 4 : -2, od = LANE & 15;
#pragma unroll
  for (int i = 0; i < 27; i++) hrow[i] = d < 9 ? (i < 9 ? E.M9[d][i] : 0.f) : (i == d ? mass_cube(d - 9) : 0.f);
  float gacc = 0.f;
  PROBE(6, stats, STAT_T_AUX3);
  // The non-empty row types go in rounds of up to HESS_TILES: each type's tile is staged in its
  // own 16 x 16 slot of E.con (free until the Cholesky), then one barrier, then the dof lanes
  // gather every tile of the round (in type order, so the sums are the same as one type at a time)
  unsigned tmask = 0;  // non-empty row types (uniform)
  for (int t = 0; t < NTYPE; t++) tmask |= E.tbase[t + 1] > E.tbase[t] ? 1u << t : 0u;
  tmask = __builtin_amdgcn_readfirstlane(tmask);
  int nst = 0, tyslots = 0;  // tiles staged in this round and their row types (4 bits each)
  auto flush = [&]() {
    if (nst == 0) return;
    SYNC();
#pragma unroll
    for (int j = 0; j < HESS_TILES; j++)
      if (j < nst) tile_gather(G + 16 * GST * j, (tyslots >> (4 * j)) & 15, bd, od, hrow, gacc);
    SYNC();
    nst = 0;
    tyslots = 0;
    PROBE(6, stats, STAT_T_AUX1);
  };
  while (tmask) {
    {
      const int t = __builtin_ctz(tmask);
      tmask &= tmask - 1u;
      const int r0 = E.tbase[t], r1 = E.tbase[t + 1];
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
      // MMX_HESS_U MFMA steps (one 4-row group each) per trip, loads first; the steps alternate
      // between the two accumulators, so each sums the same groups in the same order for any
      // MMX_HESS_U.  Types span whole groups (tbase and MMX_LDSEFC are multiples of 4), so every step
      // is full.  The LDS groups and the (rare) HBM overflow groups run in separate loops: one
      // address space per loop, no generic (flat) loads in the hot one.
      const float m_[4] = {rk == 0 ? 1.f : 0.f, rk == 1 ? 1.f : 0.f, rk == 2 ? 1.f : 0.f, rk == 3 ? 1.f : 0.f};
      const float c15 = col == 15 ? 1.f : 0.f;  // slot 15 carries g, not C B
      auto groups = [&](auto from_lds, int g_begin, int g_end) {
        constexpr bool LDS = decltype(from_lds)::value;
        float jg_[MMX_HESS_U][4], nc_[MMX_HESS_U][4], dr_[MMX_HESS_U];
        auto load_trip = [&](int s0) {
  #pragma unroll
          for (int u = 0; u < MMX_HESS_U; u++) {
            const int g0 = min(s0 + 4 * u, g_end - 4), r = g0 + rk;
            if (LDS) {
              const float4 n4 = *reinterpret_cast<const float4*>(&E.NC[g0]);  // one broadcast read
              nc_[u][0] = n4.x; nc_[u][1] = n4.y; nc_[u][2] = n4.z; nc_[u][3] = n4.w;
  #pragma unroll
              for (int m = 0; m < 4; m++) jg_[u][m] = jlds(E, g0 + m, col);  // slot 15 holds g
              dr_[u] = E.D[r];
            } else {
  #pragma unroll
              for (int m = 0; m < 4; m++) {
                jg_[u][m] = ovf_j(E, g0 + m)[col];
                nc_[u][m] = *ovf_nc(E, g0 + m);
              }
              dr_[u] = *ovf_d(E, r);
            }
          }
        };
        for (int s0 = g_begin; s0 < g_end; s0 += 4 * MMX_HESS_U) {
          float a[MMX_HESS_U], b[MMX_HESS_U];
          load_trip(s0);
  #pragma unroll
          for (int u = 0; u < MMX_HESS_U; u++) {
            // arithmetic selects over the lane's row rk (0 / 1 masks): no divergent branches
            const float live = s0 + 4 * u < g_end ? 1.f : 0.f;  // uniform
            const float* jg = jg_[u];
            const float* nc = nc_[u];
            const float own = fmaf(m_[0], jg[0], fmaf(m_[1], jg[1], fmaf(m_[2], jg[2], m_[3] * jg[3])));
            const float ncr = fmaf(m_[1], nc[1], fmaf(m_[2], nc[2], m_[3] * nc[3]));  // C_nk of row rk (0 for n)
            const float s123 = fmaf(nc[1], jg[1], fmaf(nc[2], jg[2], nc[3] * jg[3]));
            const float cpl = fmaf(ncr, jg[0], m_[0] * s123);
            a[u] = live * own;  // (slot 15 only feeds G's unused row 15)
            b[u] = live * fmaf(c15, own - fmaf(dr_[u], own, cpl), fmaf(dr_[u], own, cpl));
          }
  #pragma unroll
          for (int u = 0; u < MMX_HESS_U; u++) {
            if (u & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u], acc1, 0, 0, 0);
            else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u], acc0, 0, 0, 0);
          }
        }
      };
      const int split = min(max(r0, MMX_LDSEFC), r1);
      groups(std::true_type{}, r0, split);
      if (split < r1) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");  // the overflow rows' stores (ovf_fence)
        // group k of the type (from r0) goes to accumulator k & 1 in either loop, so the sums do not
        // depend on where the LDS rows end (the 128- and 192-row layouts are bit-identical)
        const bool odd = ((split - r0) >> 2) & 1;  // uniform
        auto swap_acc = [&]() {
          const f32x4 t = acc0;
          acc0 = acc1;
          acc1 = t;
        };
        if (odd) swap_acc();
        groups(std::false_type{}, split, r1);
        if (odd) swap_acc();
      }
      PROBE(6, stats, STAT_T_AUX0);
      // stage: lane l holds G[4 (l >> 4) + q][l & 15]
#pragma unroll
      for (int q = 0; q < 4; q++) G[16 * GST * nst + GST * (4 * rk + q) + col] = acc0[q] + acc1[q];
      tyslots |= t << (4 * nst);
      if (++nst == HESS_TILES) flush();
    }
  }
  flush();
  PROBE(6, stats, STAT_T_AUX2);
  return nd >= 0 ? gacc + mdx : 0.f;
}

// Incremental form of hess_grad_mfma for the Newton iterations after the first.  Over a line
// search only the edges whose active state flipped change their weight, so with Delta C the
// groups' change of edge-weight matrix (nonzero only in groups holding a flipped edge):
//   H_new = H_old + sum_groups B' dC B,   g_new = g_old + a H_old p + sum_groups B' dC r_new
// (g = M (x - xs) + sum B' C r; B' C_old r_new = B' C_old r_old + a B' C_old B p).  E.D / E.NC /
// slot 15 hold dC_kk, dC_nk and dC r_new (newton_wave's weight pass in delta mode); gm[q] bit 4m
// marks group m of row slice q as changed (wave-uniform).  Only the changed groups' MFMA steps run,
// and only the row types holding one are staged and gathered, LDS and HBM overflow rows alike (r05:
// with 128 LDS rows the grasp phases' rows spill; the full pass whenever rows spill, as in r02-r04,
// measured slower).  Adds into hrow; returns sum B' dC r in lane j < 27.
#define HESS_LQ (MMX_LDSEFC / WG)  // row slices held in LDS
#define HESS_NQ RPL                // row slices the delta pass covers
DEV float hess_grad_delta(EnvSh& E, float* hrow, const unsigned long long* gm) {
  float* G = lrow_of(E);
  const int col = LANE & 15, rk = LANE >> 4;
  const int nd = newton_dof(LANE);
  const int bd = nd >= 0 ? LANE >> 4 : -2, od = LANE & 15;
  const float m_[4] = {rk == 0 ? 1.f : 0.f, rk == 1 ? 1.f : 0.f, rk == 2 ? 1.f : 0.f, rk == 3 ? 1.f : 0.f};
  const float c15 = col == 15 ? 1.f : 0.f;
  float gacc = 0.f;
  int nst = 0, tyslots = 0;  // tiles staged in this round and their row types (4 bits each)
  auto flush = [&]() {
    if (nst == 0) return;
    SYNC();
#pragma unroll
    for (int j = 0; j < HESS_TILES; j++)
      if (j < nst) tile_gather(G + 16 * GST * j, (tyslots >> (4 * j)) & 15, bd, od, hrow, gacc);
    SYNC();
    nst = 0;
    tyslots = 0;
  };
  for (int t = 0; t < NTYPE; t++) {
    const int r0 = E.tbase[t], r1 = E.tbase[t + 1];
    if (r1 <= r0) continue;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    bool any = false;
#pragma unroll
    for (int q = 0; q < HESS_NQ; q++) {
      if (64 * q >= r1 || 64 * (q + 1) <= r0) continue;  // uniform
      const int lo = max(r0 - 64 * q, 0), hi = min(r1 - 64 * q, 64);
      unsigned long long m = gm[q] & (hi >= 64 ? ~0ull : ((1ull << hi) - 1ull)) & (~0ull << lo);
      if (q >= HESS_LQ && m) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");  // the HBM rows' stores
      while (m) {  // uniform: the type's changed groups, one MFMA step each
        const int g0 = 64 * q + __builtin_ctzll(m);
        m &= m - 1ull;
        any = true;
        float4 n4;
        float jg[4], dr;
        if (q < HESS_LQ) {  // (static per unrolled slice: LDS or HBM rows)
          n4 = *reinterpret_cast<const float4*>(&E.NC[g0]);
#pragma unroll
          for (int mm = 0; mm < 4; mm++) jg[mm] = jlds(E, g0 + mm, col);  // slot 15 holds dC r
          dr = E.D[g0 + rk];
        } else {
          n4 = make_float4(*ovf_nc(E, g0), *ovf_nc(E, g0 + 1), *ovf_nc(E, g0 + 2), *ovf_nc(E, g0 + 3));
#pragma unroll
          for (int mm = 0; mm < 4; mm++) jg[mm] = ovf_j(E, g0 + mm)[col];
          dr = *ovf_d(E, g0 + rk);
        }
        const float own = fmaf(m_[0], jg[0], fmaf(m_[1], jg[1], fmaf(m_[2], jg[2], m_[3] * jg[3])));
        const float ncr = fmaf(m_[1], n4.y, fmaf(m_[2], n4.z, m_[3] * n4.w));
        const float s123 = fmaf(n4.y, jg[1], fmaf(n4.z, jg[2], n4.w * jg[3]));
        const float cpl = fmaf(ncr, jg[0], m_[0] * s123);
        const float b = fmaf(c15, own - fmaf(dr, own, cpl), fmaf(dr, own, cpl));
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(own, b, acc, 0, 0, 0);
      }
    }
    if (!any) continue;
    // stage into the round's next tile; a full round (or the last type) is gathered in type order
#pragma unroll
    for (int q = 0; q < 4; q++) G[16 * GST * nst + GST * (4 * rk + q) + col] = acc[q];
    tyslots |= t << (4 * nst);
    if (++nst == HESS_TILES) flush();
  }
  flush();
  return nd >= 0 ? gacc : 0.f;
}

// ---------------------------------------------------------------- Cholesky solves of H p = v
// H is 27 x 27 and block-structured: the arm block (9 dofs) and three cube blocks (6 dofs each),
// coupled only where a constraint row spans two blocks (cpl: 4 x 4 bit mask of block pairs).
// Lanes hold rows in the Newton lane layout (hrow[i] = H[dof][i], columns in dof order); the
// solution comes back in the same layout.

// Block form (no cube-cube coupling): every cube block factors inside its own DPP row, pivots
// broadcast with row_newbcast.  Without any coupling the four blocks factor in lockstep (9 pivot
// steps for all of H; cube rows meet identity rows on their dummy lanes 6..8).  With arm-cube
// coupling the arrow order holds: the three cube blocks first (6 lockstep steps), the arm lanes
// forming their coupling columns L[arm][cube] and the Schur complement of the arm block as each
// cube pivot passes (v_readlane of the cube rows' values), then the arm block (9 steps in row 0).
// Each pivot lane collects the column of L that the transposed solve needs (c[m] = L[m][own],
// block-relative; cx[i] = L[arm i][own] for a coupled cube lane) with one select per value it
// reads anyway, so no LDS transpose.
// block-relative row of the lane: its entries in its own block's columns (dummy lanes: identity)
DEV void block_row(const float* hrow, float* hb) {
  const int r = LANE >> 4, kk = LANE & 15;
  const bool valid = r != 0 ? kk < 6 : kk < 9;
  // 0/1 masks, not selects: a select chain over hrow[m + 6 r ...] is turned into a lane-indexed
  // load, which moves hrow to scratch
  const float m0 = r == 0 ? 1.f : 0.f, m1 = r == 1 ? 1.f : 0.f, m2 = r == 2 ? 1.f : 0.f, m3 = r == 3 ? 1.f : 0.f;
#pragma unroll
  for (int m = 0; m < 9; m++) {
    const float vv = m < 6 ? fmaf(m3, hrow[21 + m], fmaf(m2, hrow[15 + m], fmaf(m1, hrow[9 + m], m0 * hrow[m]))) : m0 * hrow[m];
    hb[m] = valid ? vv : (m == kk ? 1.f : 0.f);
  }
}
// no coupling at all: the four blocks factor in lockstep (9 pivot steps; cube rows meet identity
// rows on their dummy lanes 6..8), forward solve riding along
DEV float chol_block_free(const float* hrow, float v) {
  const int r = LANE >> 4, kk = LANE & 15;
  const bool valid = r != 0 ? kk < 6 : kk < 9;
  float hb[9], c[9], dinv[9];
  block_row(hrow, hb);
#pragma unroll
  for (int m = 0; m < 9; m++) c[m] = 0.f;
  float y = valid ? v : 0.f;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const float d = fmaxf(row_bcast(hb[k], k), 1e-20f);
    const float inv = __builtin_amdgcn_rsqf(d), sd = d * inv;
    dinv[k] = inv;
    const float l = kk == k ? sd : hb[k] * inv;  // lanes after the pivot: L[own][k]
    hb[k] = l;
    const float yk = row_bcast(y, k) * inv;
    y = kk == k ? yk : (kk > k ? fmaf(-l, yk, y) : y);
#pragma unroll
    for (int m = k + 1; m < 9; m++) {
      const float lm = row_bcast(l, m);
      hb[m] = fmaf(-lm, l, hb[m]);
      c[m] = kk == k ? lm : c[m];
    }
  }
#pragma unroll
  for (int k = 8; k >= 0; k--) {  // L' z = y
    const float zk = row_bcast(y, k) * dinv[k];
    y = kk == k ? zk : (kk < k ? fmaf(-c[k], zk, y) : y);
  }
  return valid ? y : 0.f;
}
// arm-cube coupling (a grasp), no cube-cube coupling: arrow order, the three cube blocks first (6
// lockstep steps) with the arm lanes forming their coupling columns L[arm][cube] and the arm
// block's Schur complement as each cube pivot passes (v_readlane of the cube rows' values), then
// the arm block (9 steps in row 0); the transposed solve in reverse order
DEV float chol_block_arm(const float* hrow, float v, int cpla) {
  const int L = LANE, r = L >> 4, kk = L & 15;
  const bool cube = r != 0;
  const bool valid = cube ? kk < 6 : kk < 9;
  float hb[9], c[9], cx[9], dinv[9], hx[18];
  block_row(hrow, hb);
#pragma unroll
  for (int m = 0; m < 9; m++) {
    c[m] = 0.f;
    cx[m] = 0.f;
  }
#pragma unroll
  for (int m = 0; m < 18; m++) hx[m] = hrow[9 + m];  // arm lanes: the coupling columns
  float y = valid ? v : 0.f;
#pragma unroll
  for (int k = 0; k < 6; k++) {  // the cube blocks (arm lanes: l = 0, untouched)
    const float d = fmaxf(row_bcast(hb[k], k), 1e-20f);
    const float inv = __builtin_amdgcn_rsqf(d), sd = d * inv;
    dinv[k] = inv;
    const float l = cube ? (kk == k ? sd : hb[k] * inv) : 0.f;
    hb[k] = cube ? l : hb[k];
    const float yk = row_bcast(y, k) * inv;
    y = cube ? (kk == k ? yk : (kk > k ? fmaf(-l, yk, y) : y)) : y;
#pragma unroll
    for (int m = k + 1; m < 6; m++) {
      const float lm = row_bcast(l, m);
      hb[m] = fmaf(-lm, l, hb[m]);
      c[m] = cube && kk == k ? lm : c[m];
    }
#pragma unroll
    for (int b = 1; b < 4; b++) {
      if (!((cpla >> b) & 1)) continue;  // uniform
      const float invb = readlane_f(inv, 16 * b);
      const float la = cube ? 0.f : hx[6 * (b - 1) + k] * invb;  // arm lane j: L[j][cube pivot]
      hx[6 * (b - 1) + k] = la;
#pragma unroll
      for (int m = k + 1; m < 6; m++) hx[6 * (b - 1) + m] = fmaf(-readlane_f(l, 16 * b + m), la, hx[6 * (b - 1) + m]);
#pragma unroll
      for (int i = 0; i < 9; i++) {  // Schur complement of the arm block
        const float li = readlane_f(la, i);
        hb[i] = fmaf(-li, la, hb[i]);
        cx[i] = L == 16 * b + k ? li : cx[i];
      }
      y = fmaf(-la, readlane_f(y, 16 * b + k), y);  // the cube pivot's y is final
    }
  }
  if (!cube) {
#pragma unroll
    for (int k = 0; k < 9; k++) {  // the arm block, row 0
      const float d = fmaxf(row_bcast(hb[k], k), 1e-20f);
      const float inv = __builtin_amdgcn_rsqf(d), sd = d * inv;
      dinv[k] = inv;
      const float l = kk == k ? sd : hb[k] * inv;
      hb[k] = l;
      const float yk = row_bcast(y, k) * inv;
      y = kk == k ? yk : (kk > k ? fmaf(-l, yk, y) : y);
#pragma unroll
      for (int m = k + 1; m < 9; m++) {
        const float lm = row_bcast(l, m);
        hb[m] = fmaf(-lm, l, hb[m]);
        c[m] = kk == k ? lm : c[m];
      }
    }
#pragma unroll
    for (int k = 8; k >= 0; k--) {  // L' z = y: the arm block (eliminated last) first
      const float zk = row_bcast(y, k) * dinv[k];
      y = kk == k ? zk : (kk < k ? fmaf(-c[k], zk, y) : y);
    }
  }
  // the coupled cube rows take the arm's final z: the arm lanes' y no longer changes here (cx = 0 off
  // the coupled cubes), so the 9 reads are independent of the updates and issue back to back
  float za[9];
#pragma unroll
  for (int i = 0; i < 9; i++) za[i] = readlane_f(y, i);
#pragma unroll
  for (int i = 0; i < 9; i++) y = fmaf(-cx[i], za[i], y);
#pragma unroll
  for (int k = 5; k >= 0; k--) {
    const float zk = row_bcast(y, k) * dinv[k];
    y = cube ? (kk == k ? zk : (kk < k ? fmaf(-c[k], zk, y) : y)) : y;
  }
  return valid ? y : 0.f;
}

// General arrow-ordered register Cholesky (any coupling, incl. cube-cube): pivots in the order
// cube 1, cube 2, cube 3, arm, and a pivot only updates the blocks it is coupled to (cpl plus the
// fill-in eliminating a block creates among the blocks after it); cross-lane values by
// v_readlane from the dof's lane, columns of L for the transposed solve through an LDS transpose.
DEV float chol_solve_arrow(EnvSh& E, const float* hrow, float v, int cpl) {
  const int j = newton_dof(LANE);
  const int pj = j < 0 ? 1000 : (j < 9 ? j + 18 : j - 9);  // elimination position of dof j
  float h[27], dinv[27];
#pragma unroll
  for (int i = 0; i < 27; i++) h[i] = hrow[i];
#pragma unroll
  for (int pi = 0; pi < 27; pi++) {
    const int p = pi < 18 ? pi + 9 : pi - 18;
    const int bp = p < 9 ? 0 : 1 + (p - 9) / 6;
    const float d = fmaxf(readlane_f(h[p], newton_lane(p)), 1e-20f);
    const float inv = __builtin_amdgcn_rsqf(d), sd = d * inv;  // one transcendental per pivot
    dinv[p] = inv;
    const float l = j == p ? sd : h[p] * inv;  // lanes after p: L[j][p]
    h[p] = l;
#pragma unroll
    for (int B = 0; B < 4; B++) {
      const int dB = B == 0 ? 0 : 9 + 6 * (B - 1), nB = B == 0 ? 9 : 6;
      const int lastpos = B == 0 ? 26 : 6 * B - 1;  // position of the block's last pivot
      if (lastpos <= pi) continue;                    // block already eliminated (static)
      if (B == bp || ((cpl >> (4 * bp + B)) & 1)) {
#pragma unroll
        for (int k = 0; k < nB; k++) {
          const int i = dB + k;
          const int qi = i < 9 ? i + 18 : i - 9;
          if (qi > pi) h[i] = fmaf(-readlane_f(l, newton_lane(i)), l, h[i]);
        }
      }
    }
    const bool last_of_block = pi == 5 || pi == 11 || pi == 17;
    if (last_of_block) {  // fill-in among the blocks eliminated later (cubes after bp, then arm)
#pragma unroll
      for (int x = 0; x < 4; x++)
#pragma unroll
        for (int yb = 0; yb < 4; yb++) {
          const bool later_x = x == 0 || x > bp, later_y = yb == 0 || yb > bp;
          if (x != yb && later_x && later_y && x != bp && yb != bp && ((cpl >> (4 * bp + x)) & 1) &&
              ((cpl >> (4 * bp + yb)) & 1))
            cpl |= 1 << (4 * x + yb);
        }
    }
  }
  float y = j >= 0 ? v : 0.f;
#pragma unroll
  for (int pi = 0; pi < 27; pi++) {  // L y = v in elimination order
    const int p = pi < 18 ? pi + 9 : pi - 18;
    const float yk = readlane_f(y, newton_lane(p)) * dinv[p];
    y = j == p ? yk : (pj > pi ? fmaf(-h[p], yk, y) : y);
  }
  const int jc = max(j, 0);
  if (j >= 0) {
#pragma unroll
    for (int m = 0; m < 27; m++) arrow_of(E)[27 * j + m] = h[m];
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // (HBM: the stores complete before the reads)
  SYNC();
  float c[27];
#pragma unroll
  for (int k = 0; k < 27; k++) c[k] = arrow_of(E)[27 * k + jc];  // L[k][j]
#pragma unroll
  for (int pi = 26; pi >= 0; pi--) {  // L' z = y
    const int p = pi < 18 ? pi + 9 : pi - 18;
    const float zk = readlane_f(y, newton_lane(p)) * dinv[p];
    y = j == p ? zk : (pj < pi ? fmaf(-c[p], zk, y) : y);
  }
  SYNC();
  return j >= 0 ? y : 0.f;
}

// H^{-1} v: the block form unless two cubes are coupled (a cube resting on or pushing another).
// The general solve stays inline although no C3 episode reaches it (tests/test_cube_contact_kat.py
// does): out of line (its Hessian row by value, no register save on either side) the kernel is ~3,100
// instructions shorter but no faster (-0.01 % on the medians, the spread 0.3 %: profiles/r07_ab_nocsr.json).
DEV float chol_solve(EnvSh& E, const float* hrow, float v, int cpl) {
  float* stats = E.stats;
  CLK_DECL;
  const bool cube_cube = (cpl & 0x6AC0) != 0;  // bits 4 x + y with x, y in 1..3, x != y
  const float y = cube_cube ? chol_solve_arrow(E, hrow, v, cpl)
                            : ((cpl & 0xE) ? chol_block_arm(hrow, v, cpl & 0xE) : chol_block_free(hrow, v));
  // probe set 9: cycles of the uncoupled / arm-coupled / cube-cube solves; AUX3 counts the
  // arm-coupled solves + 1000 x the cube-cube ones
  PROBE(9, stats, cube_cube ? STAT_T_AUX1 : ((cpl & 0xE) ? STAT_T_AUX2 : STAT_T_AUX0));
  if (MMX_PROBE == 9 && LANE == 0) stats[STAT_T_AUX3] += cube_cube ? 1000.f : ((cpl & 0xE) ? 1.f : 0.f);
  return y;
}

// exit: 0 converged (gradient below tol), 1 no progress (step below 1e-9 with the gradient above
// tol: an fp32 stall), 2 iteration cap reached above tol
DEV int newton_wave(EnvSh& E, int max_iter, float tol, float& resid, int& exit, const float* mu_in) {
  float* stats = E.stats;
  CLK_DECL;
  const int nefc = E.nefc, nsingle = E.nsingle;
  // per owned row: D (1/R; the contact's common pyramid R), mu (from the row build, in registers) and
  // the edge coefficients
  float dd[RPL], mu[RPL];
#pragma unroll
  for (int q = 0; q < RPL; q++) {
    const int i = LANE + WG * q;
    dd[q] = i < nefc ? dget(E, i) : 0.f;
    mu[q] = i < nefc ? mu_in[q] : 0.f;
  }
  // start from the cheaper of the warm start and qacc_smooth (as MuJoCo does)
  float c_ws, c_s, ra[RPL], rs[RPL], mws, ms;
  cost2_wave(E, E.x, E.qacc_s, mu, dd, c_ws, c_s, ra, rs, mws, ms);
  const bool from_ws = c_ws < c_s;
  const int nd = newton_dof(LANE);  // the lane's dof in the Newton lane layout (-1: none)
  if (nd >= 0) E.x[nd] = from_ws ? E.x[nd] : E.qacc_s[nd];
  float mdx = from_ws ? mws : ms;  // (M (x - xs))_lane, kept current through the iterations
  float scale = nd >= 0 ? E.qfrc[nd] * E.qfrc[nd] : 0.f;
  scale = sqrtf(wave_sum(scale)) + 1.f;
  float rr[RPL], jp[RPL];  // basis-row residuals J x - aref and J p
#pragma unroll
  for (int q = 0; q < RPL; q++) {
    rr[q] = from_ws ? ra[q] : rs[q];
    jp[q] = 0.f;
  }
  int cpl = 0;  // block pairs that share constraint rows (uniform)
  for (int t = 0; t < NTYPE; t++)
    if (kTB1[t] != BLK_NONE && E.tbase[t + 1] > E.tbase[t]) cpl |= (1 << (4 * kTB0[t] + kTB1[t])) | (1 << (4 * kTB1[t] + kTB0[t]));
  cpl = __builtin_amdgcn_readfirstlane(cpl);
  SYNC();
  int it = 0;
  resid = 0.f;
  exit = 2;
  // Hessian rows and gradient persist across iterations: after the first full pass each later one
  // adds only the groups whose edge weights changed (hess_grad_delta); act holds the lane's edge
  // active bits (bit 2q: edge 0 of slice q, bit 2q + 1: edge 1) the current H was built from
  float hrow[32];
  float gpred = 0.f;  // g_old + a H_old p: the gradient at the new point before the weight change
  int act = 0;
  PROBE(1, stats, STAT_T_AUX3);
  for (; it < max_iter; it++) {
    // per group: the edge-weight matrix C (C_kk -> D, C_nk -> NC) and g = sum_e w_e r_e c_e
    // (-> slot 15), from the active edges of the current residuals; a contact's normal row
    // collects its edges' normal parts over the DPP quad.  Delta mode: the same with the change
    // of each edge's weight (+-D where its active state flipped, else 0), and a mask of the
    // groups holding a flipped edge.
    const bool delta = it > 0;  // uniform
    unsigned long long gm[HESS_NQ];
#pragma unroll
    for (int q = 0; q < HESS_NQ; q++) gm[q] = 0ull;
#pragma unroll
    for (int q = 0; q < RPL; q++) {
      if (WG * q >= nefc) break;  // uniform: no rows past this slice
      const int i = LANE + WG * q;
      const EdgeCoef ec = edge_coef(i, nefc, nsingle, mu[q]);
      const float rn = quad_first(rr[q]);
      const float e0 = fmaf(ec.a0, rn, ec.b0 * rr[q]), e1 = fmaf(ec.a1, rn, ec.b1 * rr[q]);
      const bool on0 = EQROW(q) || e0 < 0.f, on1 = e1 < 0.f;  // (missing edges: coefficients 0)
      const bool was0 = (act >> (2 * q)) & 1, was1 = (act >> (2 * q + 1)) & 1;
      act = (act & ~(3 << (2 * q))) | ((on0 ? 1 : 0) << (2 * q)) | ((on1 ? 2 : 0) << (2 * q));
      float w0 = on0 ? dd[q] : 0.f, w1 = on1 ? dd[q] : 0.f;
      if (delta) {
        w0 = on0 == was0 ? 0.f : (on0 ? dd[q] : -dd[q]);
        w1 = on1 == was1 ? 0.f : (on1 ? dd[q] : -dd[q]);
        if (q < HESS_NQ) {
          const unsigned long long bm = __ballot(w0 != 0.f || w1 != 0.f);
          gm[q < HESS_NQ ? q : 0] = (bm | (bm >> 1) | (bm >> 2) | (bm >> 3)) & 0x1111111111111111ull;
        }
      }
      const float ckk = fmaf(w0 * ec.b0, ec.b0, w1 * ec.b1 * ec.b1);
      const float cnk = fmaf(w0 * ec.a0, ec.b0, w1 * ec.a1 * ec.b1);
      const float gk = fmaf(w0 * e0, ec.b0, w1 * e1 * ec.b1);
      const float cnn = quad_sum(fmaf(w0 * ec.a0, ec.a0, w1 * ec.a1 * ec.a1));
      const float gn = quad_sum(fmaf(w0 * e0, ec.a0, w1 * e1 * ec.a1));
      const bool nrow = i >= nsingle && (i & 3) == 0;
      if (i < nefc) {
        jset(E, i, 15, nrow ? gn : gk);  // g for the gradient (the row's aref slot is dead after the setup)
        dset(E, i, nrow ? cnn : ckk);    // C diagonal (D itself is in registers since the setup)
        ncset(E, i, nrow ? 0.f : cnk);
      }
    }
    ovf_fence(nefc);
    SYNC();
    PROBE(1, stats, STAT_T_AUX0);
    float g;
    if (delta) {
      g = gpred + hess_grad_delta(E, hrow, gm);
    } else {
      g = hess_grad_mfma(E, nefc, hrow, mdx);
    }
    resid = sqrtf(wave_sum(g * g)) / scale;
    PROBE(1, stats, STAT_T_AUX1);
    if (resid < tol) {
      exit = 0;
      break;
    }
    const float pj = chol_solve(E, hrow, -g, cpl);
    if (nd >= 0) E.p[nd] = pj;
    SYNC();
    float hp = 0.f;  // (H p)_lane: the gradient's change per unit step while no edge changes state
#pragma unroll
    for (int m = 0; m < 27; m++) hp = fmaf(hrow[m], E.p[m], hp);
    PROBE(1, stats, STAT_T_AUX2);
    // exact line search on phi(a) = cost(x + a p): phi' is piecewise linear and increasing; per
    // owned row its (up to two) edges e(a) = e + a je
    float e0[RPL], e1[RPL], j0[RPL], j1[RPL];
#pragma unroll
    for (int q = 0; q < RPL; q++) {
      e0[q] = e1[q] = j0[q] = j1[q] = 0.f;
      jp[q] = 0.f;
      if (WG * q >= nefc) continue;  // uniform: the slice holds no row
      const int i = LANE + WG * q;
      jp[q] = i < nefc ? row_dot16(E, i, E.p) : 0.f;
      const EdgeCoef ec = edge_coef(i, nefc, nsingle, mu[q]);
      const float rn = quad_first(rr[q]), pn = quad_first(jp[q]);
      e0[q] = fmaf(ec.a0, rn, ec.b0 * rr[q]);
      e1[q] = fmaf(ec.a1, rn, ec.b1 * rr[q]);
      j0[q] = fmaf(ec.a0, pn, ec.b0 * jp[q]);
      j1[q] = fmaf(ec.a1, pn, ec.b1 * jp[q]);
    }
    PROBE(10, stats, STAT_T_AUX0);
    float c0 = 0.f, c1 = 0.f, mp = 0.f;
    if (nd >= 0) {
      mp = mass_mul(E, E.p);
      c0 = mp * (E.x[nd] - E.qacc_s[nd]);
      c1 = mp * pj;
    }
    c0 = wave_sum(c0);
    c1 = wave_sum(c1);
    PROBE(10, stats, STAT_T_AUX1);
    // the lane's edge active bits at step a, laid out like `act` (bit 2q: edge 0 of slice q, with
    // the equality row always on; bit 2q + 1: edge 1)
    auto act_at = [&](float a) {
      int b = 0;
#pragma unroll
      for (int q = 0; q < RPL; q++) {
        if (WG * q >= nefc) break;  // uniform
        b |= ((EQROW(q) || fmaf(a, j0[q], e0[q]) < 0.f) ? 1 : 0) << (2 * q);
        b |= (fmaf(a, j1[q], e1[q]) < 0.f ? 2 : 0) << (2 * q);
      }
      return b;
    };
    // phi' is linear on any interval over which no edge changes state (each edge is linear in a),
    // so a Newton root of phi' whose active set equals the set of the point it was taken from is
    // the minimiser and needs no confirming evaluation (which would only move it by rounding).  The
    // first evaluation, at the full step a = 1, always runs: it corrects the step length for the
    // fp32 error of the Cholesky solve p (accepting a = 1 unevaluated moved whole C3 episodes by
    // up to 7e-4 m against the solver at MuJoCo's tolerance).
    float alpha = 1.f, lo = 0.f, hi = 3e38f;
    int bcur = act_at(1.f);
    bool exact = false;  // (+1.0 % env steps/s in the A/B, DESIGN §2)
    for (int ls = 0; ls < 24 && !exact; ls++) {
      if (MMX_PROBE == 10 && LANE == 0) stats[STAT_T_AUX3] += 1.f;  // line-search steps
      float d1 = 0.f, d2 = 0.f;
#pragma unroll
      for (int q = 0; q < RPL; q++) {
        if (WG * q >= nefc) break;  // uniform
        const float a0 = fmaf(alpha, j0[q], e0[q]), a1 = fmaf(alpha, j1[q], e1[q]);
        const float s0 = EQROW(q) || a0 < 0.f ? dd[q] * j0[q] : 0.f;
        const float s1 = a1 < 0.f ? dd[q] * j1[q] : 0.f;
        d1 = fmaf(s0, a0, fmaf(s1, a1, d1));
        d2 = fmaf(s0, j0[q], fmaf(s1, j1[q], d2));
      }
      d1 = wave_sum(d1) + c0 + alpha * c1;
      d2 = wave_sum(d2) + c1;
      if (d1 < 0.f) lo = alpha;
      else hi = alpha;
      float na = alpha - d1 / fmaxf(d2, 1e-30f);
      const bool newton = na >= lo && na <= hi;
      if (!newton) na = hi < 3e38f ? 0.5f * (lo + hi) : 2.f * alpha;
      if (fabsf(na - alpha) <= 1e-6f * fabsf(alpha) + 1e-12f) {
        alpha = na;
        break;
      }
      const int bn = act_at(na);
      exact = newton && __ballot(bn != bcur) == 0ull;
      bcur = bn;
      alpha = na;
    }
    PROBE(1, stats, STAT_T_AUX3);
    PROBE(10, stats, STAT_T_AUX2);
    float stepn = 0.f;
    if (nd >= 0) {
      E.x[nd] += alpha * pj;
      stepn = alpha * alpha * pj * pj;
    }
    mdx = fmaf(alpha, mp, mdx);
    bool flip = false;  // an edge changed active state over the step
#pragma unroll
    for (int q = 0; q < RPL; q++) {
      if (WG * q >= nefc) break;  // uniform
      const float a0 = fmaf(alpha, j0[q], e0[q]), a1 = fmaf(alpha, j1[q], e1[q]);
      flip |= !EQROW(q) && ((a0 < 0.f) != (e0[q] < 0.f));
      flip |= (a1 < 0.f) != (e1[q] < 0.f);
      rr[q] = fmaf(alpha, jp[q], rr[q]);
    }
    SYNC();
    stepn = sqrtf(wave_sum(stepn));
    if (stepn < 1e-9f) {
      it++;
      exit = 1;
      break;
    }
    gpred = nd >= 0 ? fmaf(alpha, hp, g) : 0.f;
    if (__ballot(flip) == 0ull) {
      // same active set: H is unchanged, so g(x + a p) = g + a H p exactly; when that already
      // meets the tolerance the confirming Hessian pass is skipped
      const float rn = sqrtf(wave_sum(gpred * gpred)) / scale;
      if (rn < tol) {
        resid = rn;
        it++;
        exit = 0;
        break;
      }
    }
  }
  SYNC();
  return it;
}

#undef LANE
#define LANE ((int)(threadIdx.x & 63))
