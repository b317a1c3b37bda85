// Part 3 of mmx_step.inc (an ordered fragment, included there and nowhere else): collision detection in three
// passes, so that the 192-row layout can run them on two waves: collide_prune (geom poses, the persistent
// broadphase list, the sphere / plane test, the candidates by pair class), collide_pairs (the narrowphase of
// mmx_geom.h per class; `which` picks the env wave's classes, the helper wave's, or all) and collide_sort (the
// contacts by key); collide_wave is all three on one wave.  Relies on the lds part (the contact record, the
// COL_* scratch map, the wave primitives) and on arm_body_speed of the dynamics part.
// ============================================================================ collision (wave)
DEV Geom geom_pose(const EnvSh& E, int g) {
  Geom G;
  G.g = g;
  G.type = MMX_geom_type[g];
  const int b = MMX_geom_body[g];
  if (MMX_body_static[b]) {
    G.x = V3{MMX_geom_static_xpos[3 * g], MMX_geom_static_xpos[3 * g + 1], MMX_geom_static_xpos[3 * g + 2]};
#pragma unroll
    for (int k = 0; k < 9; k++) G.R.m[k] = MMX_geom_static_xmat[9 * g + k];
  } else {
    const V3 bx = body_x(E, b);
    const M3 bR = body_R(E, b);
    G.x = bx + mul(bR, V3{MMX_geom_pos[3 * g], MMX_geom_pos[3 * g + 1], MMX_geom_pos[3 * g + 2]});
    M3 Lm;
#pragma unroll
    for (int k = 0; k < 9; k++) Lm.m[k] = MMX_geom_lmat[9 * g + k];
    G.R = mul(bR, Lm);
  }
  return G;
}

// appends contacts to the env's LDS list; key = pair index * 8 + local sequence gives a
// deterministic contact order independent of lane timing
struct WaveSink {
  EnvSh* E;
  int key;
  bool store;
  bool ro;
  int geoms;  // the geoms packed above the order key: g1 << 16 | g2 << 22
  int key0;
  DEV WaveSink(EnvSh* e, int p, bool st, int g1, int g2) : E(e), key(p * 8), store(st) {
    key0 = p * 8;
    geoms = (g1 << 16) | (g2 << 22);
    const int c1 = MMX_geom_class[g1], c2 = MMX_geom_class[g2];
    ro = (c1 == 1 && c2 == 2) || (c1 == 2 && c2 == 1);
  }
  DEV void add(int g1, int g2, float dist, V3 pos, V3 nrm) { put(reserve(1), g1, g2, dist, pos, nrm); }
  // contact `order` of the pair (its key = pair * 8 + order, as the sequential put would give it)
  // into a reserved slot: the lane-group form of the box-box narrowphase puts a pair's contacts
  // from several lanes at once
  DEV void put_at(int slot, int order, int g1, int g2, float dist, V3 pos, V3 nrm) {
    key = key0 + order;
    put(slot, g1, g2, dist, pos, nrm);
  }
  // n consecutive contact slots with one LDS atomic (a pair's corners / clipped points are
  // counted first, then reserved together); returns the first slot, MMX_MAXCON when none is kept
  DEV int reserve(int n) {
    if (n <= 0) return MMX_MAXCON;
    if (ro) atomicOr(&E->flags, (int)SHF_ROBOT_OBST);
    if (!store) return MMX_MAXCON;
    const int slot = atomicAdd(&E->ncon, n);
    if (slot + n > MMX_MAXCON) atomicOr(&E->flags, (int)SHF_CON_OVF);
    return slot;
  }
  // contact into a reserved slot (slots past the list are dropped); keys follow the call order
  DEV void put(int slot, int g1, int g2, float dist, V3 pos, V3 nrm) {
    if (slot >= MMX_MAXCON) return;
    nrm = normalize(nrm);
    const CRecW c{scr_of(*E) + COL_CON, slot};
    c[CL_DIST] = dist;
    c[CL_POS] = pos.x; c[CL_POS + 1] = pos.y; c[CL_POS + 2] = pos.z;
    c[CL_N] = nrm.x; c[CL_N + 1] = nrm.y; c[CL_N + 2] = nrm.z;
    c[CL_KEY] = __int_as_float((key++) | geoms);
  }
};

DEV V3 geom_half(const float* gx, int g) {
  const float* o = gx + GXS * g;
  return V3{o[GX_HALF], o[GX_HALF + 1], o[GX_HALF + 2]};
}
DEV Geom geom_lds(const float* gx, int g) {
  const float* o = gx + GXS * g;
  Geom G;
  G.g = g;
  G.type = __float_as_int(o[GX_TYPE]);
  G.x = V3{o[0], o[1], o[2]};
#pragma unroll
  for (int k = 0; k < 9; k++) G.R.m[k] = o[3 + k];
  return G;
}
// MMX_pair_packed[p]: the geoms of pair p ordered by type (plane first), as the narrowphase dispatch
// expects (pre-sorted by the model compiler).  A candidate entry carries the pair index and both geom ids (p | g1 << 12 | g2 << 18), so the
// passes after the sphere test decode them from LDS instead of gathering MMX_pair_packed (a
// per-lane global-memory load) again.  Classes go above bit 24 (collide_prune's regrouping).
static_assert(MMX_NPAIR < 4096 && MMX_NGEOM <= 64, "candidate entry packing");
DEV int cand_pack(int p, int pk) { return p | ((pk & 255) << 12) | ((pk >> 8) << 18); }
DEV void cand_unpack(int e, int& p, int& g1, int& g2) {
  p = e & 4095;
  g1 = (e >> 12) & 63;
  g2 = (e >> 18) & 63;
}
DEV bool robot_obstacle(int g1, int g2) {
  const int c1 = MMX_geom_class[g1], c2 = MMX_geom_class[g2];
  return (c1 == 1 && c2 == 2) || (c1 == 2 && c2 == 1);
}
// stream compaction of one wave's flags into list[base...]; returns the new length
DEV int wave_compact(bool keep, int* list, int base, int val) {
  const unsigned long long m = __ballot(keep);
  const int pos = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
  if (keep) list[base + pos] = val;
  return base + __popcll(m);
}

// Collision in coherent stages: (1) world poses of all geoms into LDS, one lane per geom;
// (2) bounding-sphere / plane-distance prune of all pairs, compacted with ballots; (3) OBB prune,
// split by narrowphase class into per-class lists (E.ncls); (4) one pass per class (plane-convex
// / box lane per pair, box-box one pair per lane quad, GJK/EPA one pair per wave), so lanes of a
// pass run the same code; (5) deterministic rank sort of the contacts by pair key.  Every prune is
// conservative, so the contact set equals the all-pairs narrowphase.
// The persistent list's displacement bound after this substep: E.cdisp + 1.25 x 2 dt x the largest
// |origin velocity| + |angular velocity| x crad over the moving bodies (+ 1e-5), from qvel and THIS
// substep's kinematics.  arm: the lane's arm-body speed (body_speed_exact).  The one-wave build passes
// the RNE's maximum (E.cspd: the dynamics ran before the prune); in the two-wave build the env wave
// computes the speeds itself (arm_body_speed), so it reads nothing the helper wave writes between
// barriers A and P.  Lanes 10..12 take the cubes' free joints.  The same bits in both compiles (see
// sv_fma_exact): the two layouts keep, or rebuild, the list in the same substeps.
DEV float list_disp_next(const EnvSh& E, float arm) {
#pragma clang fp reassociate(off) contract(off)
  float s = arm;
  if (LANE >= 10 && LANE < 13) {
    const float* v = E.qvel + 9 + 6 * (LANE - 10);
    s = fmaf(sqrtf(fmaf(v[3], v[3], fmaf(v[4], v[4], v[5] * v[5]))), E.crad,
             sqrtf(fmaf(v[0], v[0], fmaf(v[1], v[1], v[2] * v[2]))));
  }
  return E.cdisp + fmaf(1.25f * 2.f * kDt, wave_max(s), 1e-5f);
}

DEV void collide_prune(EnvSh& E, bool only_ro) {
  float* stats = E.stats;
  CLK_DECL;
  if (LANE == 0) {
    E.ncon = 0;
    E.flags &= ~SHF_ROBOT_OBST;  // (SHF_CON_OVF is sticky from the record load to the fold: any substep's overflow counts)
  }
  float* scr = scr_of(E);
  float* gx = scr + COL_GX;
  int* cand = reinterpret_cast<int*>(scr + COL_CAND);
  // (2) runs over the persistent list when it is still valid: its pairs were within
  // MMX_CAND_MARGIN of contact at the build, and no pair has since closed by more than the bound
  // cdisp = sum over substeps of 2 dt max over bodies (origin speed + angular speed x crad) (x 1.25
  // for the integrators' second-order terms; list_disp_next).  The list is in pair order, so the exact test below
  // keeps the same candidates, in the same order, as the all-pairs pass.
  bool use_list = false;
  if (!only_ro && E.ncand >= 0) {
#if MMX_STEP_HELPER
    const float nd = list_disp_next(E, arm_body_speed(E));
#else
    const float nd = list_disp_next(E, LANE < 10 ? E.cspd : 0.f);
#endif
    use_list = nd < 0.5f * MMX_CAND_MARGIN;
    SYNC();
    if (LANE == 0 && use_list) E.cdisp = nd;
  }
  const bool rebuild = !only_ro && !use_list;
  if (LANE < MMX_NGEOM) {
    const Geom G = geom_pose(E, LANE);
    float* o = gx + GXS * LANE;
    o[0] = G.x.x; o[1] = G.x.y; o[2] = G.x.z;
#pragma unroll
    for (int k = 0; k < 9; k++) o[3 + k] = G.R.m[k];
    o[GX_RB] = MMX_geom_rbound[LANE];
    o[GX_TYPE] = __int_as_float(G.type);
    o[GX_HALF] = MMX_geom_aabb[3 * LANE];  // bounding-box half extents in the geom frame (= size for boxes)
    o[GX_HALF + 1] = MMX_geom_aabb[3 * LANE + 1];
    o[GX_HALF + 2] = MMX_geom_aabb[3 * LANE + 2];
  }
  if (rebuild) {  // uniform: the moving geoms' extent about their body origins (rigid: any pose)
    float ext = 0.f;
    if (LANE < MMX_NGEOM) {
      const int b = MMX_geom_body[LANE];
      if (!MMX_body_static[b]) ext = norm(V3{gx[GXS * LANE], gx[GXS * LANE + 1], gx[GXS * LANE + 2]} - body_x(E, b)) +
                                     MMX_geom_rbound[LANE];
    }
    ext = wave_max(ext);
    if (LANE == 0) E.crad = ext;
  }
  SYNC();
  PROBE(2, stats, STAT_T_AUX0);
  // (2) sphere / plane-distance prune
  auto sphere_test = [&](int p, int pk, float infl) {
    const int g1 = pk & 255, g2 = pk >> 8;
    if (only_ro && !robot_obstacle(g1, g2)) return false;
    const float* o1 = gx + GXS * g1;
    const float* o2 = gx + GXS * g2;
    const V3 d = V3{o2[0] - o1[0], o2[1] - o1[1], o2[2] - o1[2]};
    if (__float_as_int(o1[GX_TYPE]) == GT_PLANE) return d.x * o1[5] + d.y * o1[8] + d.z * o1[11] <= o2[GX_RB] + infl;
    const float rb = o1[GX_RB] + o2[GX_RB] + infl;
    return dot(d, d) <= rb * rb;
  };
  int nc = 0;
  if (use_list) {  // uniform: the list's pairs only (<= MMX_CAND_CAP, pair order; in the overflow block)
    const int n = E.ncand;
    constexpr int NLP = (MMX_CAND_CAP + WG - 1) / WG;
    int lp[NLP], lk[NLP];  // every pass's pair-table gather in flight at once
    const unsigned short* cl = cand_of(E);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");  // the rebuild's stores (below)
#pragma unroll
    for (int q = 0; q < NLP; q++) {
      const int k = q * WG + LANE;
      lp[q] = k < n ? (int)cl[k] : 0;
      lk[q] = WG * q < n ? MMX_pair_packed[lp[q]] : 0;
    }
#pragma unroll
    for (int q = 0; q < NLP; q++) {
      if (WG * q >= n) break;  // uniform
      const int k = q * WG + LANE;
      const bool keep = k < n && sphere_test(lp[q], lk[q], 0.f);
      nc = wave_compact(keep, cand, nc, cand_pack(lp[q], lk[q]));
    }
  } else {
  // all pairs: unrolled so the pair-table loads issue together
  constexpr int NPASS = (MMX_NPAIR + WG - 1) / WG;
  int pg[NPASS];  // all pair-table loads in flight at once
#pragma unroll
  for (int q = 0; q < NPASS; q++) {
    const int p = min(q * WG + LANE, MMX_NPAIR - 1);
    pg[q] = MMX_pair_packed[p];
  }
  // all tests first (ballot masks in SGPRs), compaction stores after: no LDS store between the
  // passes' gathers, so the compiler may keep several passes' loads in flight
  unsigned long long km[NPASS], ki[NPASS];
#pragma unroll
  for (int q = 0; q < NPASS; q++) {
    const int p = q * WG + LANE;
    km[q] = __ballot(p < MMX_NPAIR && sphere_test(p, pg[q], 0.f));
    ki[q] = rebuild ? __ballot(p < MMX_NPAIR && sphere_test(p, pg[q], MMX_CAND_MARGIN)) : 0ull;
  }
  int ni = 0;
#pragma unroll
  for (int q = 0; q < NPASS; q++) {
    const unsigned long long m = km[q];
    if ((m >> LANE) & 1ull) {
      const int pos = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      if (nc + pos < COL_LIST) cand[nc + pos] = cand_pack(q * WG + LANE, pg[q]);
    }
    nc += __popcll(m);
    if (rebuild) {  // the inflated set -> the persistent list (pair order)
      const unsigned long long mi = ki[q];
      const int pos = __builtin_amdgcn_mbcnt_hi((unsigned)(mi >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mi, 0u));
      if (((mi >> LANE) & 1ull) && ni + pos < MMX_CAND_CAP) cand_of(E)[ni + pos] = (unsigned short)(q * WG + LANE);
      ni += __popcll(mi);
    }
  }
  if (rebuild) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the list's stores complete before its next read
    if (LANE == 0) {
      E.ncand = ni <= MMX_CAND_CAP ? ni : -1;
      E.cdisp = 0.f;
    }
  }
  if (nc > COL_LIST) {  // uniform: more sphere-test survivors than the list holds (flagged; none in C3)
    if (LANE == 0) E.flags |= SHF_CON_OVF;
    nc = COL_LIST;
  }
  }
  SYNC();
  PROBE(2, stats, STAT_T_AUX1);
  // (3) OBB prune and class (0 plane, 1 box-box, 2 GJK, 3 pruned); then the candidates are
  // regrouped in place as [plane | box-box | GJK], each group in candidate (pair) order
  constexpr int NCP = (COL_LIST + WG - 1) / WG;
  int ce[NCP];
  int ncls[3] = {0, 0, 0};
#pragma unroll
  for (int q = 0; q < NCP; q++) {
    const int k = q * WG + LANE;
    int c = 3, p = 0;
    if (q * WG < nc) {
      if (k < nc) {
        p = cand[k];
        int pp, g1, g2;
        cand_unpack(p, pp, g1, g2);
        const Geom A = geom_lds(gx, g1), B = geom_lds(gx, g2);
        if (A.type == GT_PLANE) c = 0;
        else if (obb_overlap(A, B, geom_half(gx, g1), geom_half(gx, g2))) c = (A.type == GT_BOX && B.type == GT_BOX) ? 1 : 2;
      }
#pragma unroll
      for (int t = 0; t < 3; t++) ncls[t] += __popcll(__ballot(c == t));
    }
    ce[q] = p | (c << 24);  // (p: the packed candidate entry, 24 bits)
  }
  SYNC();
  int base[3] = {0, ncls[0], ncls[0] + ncls[1]};
#pragma unroll
  for (int q = 0; q < NCP; q++) {
    if (q * WG < nc) {
      const int c = ce[q] >> 24;
#pragma unroll
      for (int t = 0; t < 3; t++) base[t] = wave_compact(c == t, cand, base[t], ce[q] & 0xFFFFFF);
    }
  }
  if (LANE == 0) {
    E.ncls[0] = ncls[0];
    E.ncls[1] = ncls[1];
    E.ncls[2] = ncls[2];
  }
  SYNC();
  if (MMX_PROBE == 4 && LANE == 0) {
    stats[STAT_T_AUX0] += (float)nc;
    stats[STAT_T_AUX1] += (float)ncls[1];
    stats[STAT_T_AUX2] += (float)ncls[2];
    stats[STAT_T_AUX3] += (float)ncls[0];
  }
  // probe set 13 (VERDICT r05 item 3): per collision pass of a substep, the full 780-pair prunes (no
  // valid persistent list), the list rebuilds that then kept no list (more than MMX_CAND_CAP pairs),
  // and the box-box / GJK candidates after the OBB prune
  if (MMX_PROBE == 13 && LANE == 0 && !only_ro) {
    stats[STAT_T_AUX0] += use_list ? 0.f : 1.f;
    stats[STAT_T_AUX1] += (rebuild && E.ncand < 0) ? 1.f : 0.f;
    stats[STAT_T_AUX2] += (float)ncls[1];
    stats[STAT_T_AUX3] += (float)ncls[2];
  }
  // probe set 14 (the delay builds; no phase clock needed): the full prunes, and the list's displacement
  // bound as this pass leaves it, so the list-use decisions and the speeds they used show in the stats
  if (MMX_PROBE == 14 && LANE == 0 && !only_ro) {
    stats[STAT_T_AUX0] += use_list ? 0.f : 1.f;
    stats[STAT_T_AUX1] = E.cdisp;
  }
  // probe set 16 (sizes the axis cache, mmx_gjk_cache.h): the most GJK candidates one collision pass of this env
  // has had (a maximum: read from the env's stats, tools/gpu_probe.py gjk_dist, not from the per-phase sums), and
  // the passes with more than 2, 4 and MMX_AXIS_SLOTS of them
  if (MMX_PROBE == 16 && LANE == 0 && !only_ro) {
    stats[STAT_T_AUX0] = fmaxf(stats[STAT_T_AUX0], (float)ncls[2]);
    stats[STAT_T_AUX1] += ncls[2] > 2 ? 1.f : 0.f;
    stats[STAT_T_AUX2] += ncls[2] > 4 ? 1.f : 0.f;
    stats[STAT_T_AUX3] += ncls[2] > MMX_AXIS_SLOTS ? 1.f : 0.f;
  }
  PROBE(2, stats, STAT_T_AUX2);
  PROBE(5, stats, STAT_T_AUX3);
}

// (4) narrowphase over the class lists of collide_prune: which & 1 = plane pairs and box-box
// pairs (lane per pair), which & 2 = GJK/EPA pairs (the whole wave on one pair at a time, EPA
// polytope in LDS beside the box-box polygons)
DEV void collide_pairs(EnvSh& E, bool only_ro, int which) {
  float* stats = E.stats;
  CLK_DECL;
  float* scr = scr_of(E);
  const float* gx = scr + COL_GX;
  const int* cand = reinterpret_cast<const int*>(scr + COL_CAND);
  const int n0 = E.ncls[0], n1 = E.ncls[1], n2 = E.ncls[2];
  // the axis cache's entries, one per lane, loaded before the lane-per-pair passes so that they have arrived when
  // the first GJK pair asks (the one-wave layout; the helper wave has only the barrier before it).  The
  // robot-obstacle pass of the step end runs without the cache: in the two-wave layout the env wave runs its GJK
  // pairs, and an entry is only ever touched by one lane of one wave, the one that runs the substeps' GJK class.
  AxisCache ac;
  if (MMX_GJK_CACHE && (which & 2) && !only_ro && n2 > 0) axis_cache_load(ac, axis_of(E));  // uniform
  if (which & 1) {
    for (int k = LANE; k < n0; k += WG) {  // plane-box / plane-convex
      int p, g1, g2;
      cand_unpack(cand[k], p, g1, g2);
      const Geom A = geom_lds(gx, g1), B = geom_lds(gx, g2);
      WaveSink cs(&E, p, !only_ro, g1, g2);
      if (B.type == GT_BOX) plane_box(cs, A, B, geom_half(gx, g2));
      else if (B.type == GT_MESH) plane_convex(cs, A, B);
    }
    SYNC();
    PROBE(5, stats, STAT_T_AUX0);
    // box-box, one pair per lane quad (16 pairs per pass): the clip's vertices split over the quad
    V3* poly = reinterpret_cast<V3*>(scr + COL_WORK + COL_POLY * (LANE >> 2));
    for (int k0 = 0; k0 < n1; k0 += WG / 4) {
      const int k = k0 + (LANE >> 2);
      if (k < n1) {
        int p, g1, g2;
        cand_unpack(cand[n0 + k], p, g1, g2);
        const Geom A = geom_lds(gx, g1), B = geom_lds(gx, g2);
        WaveSink cs(&E, p, !only_ro, g1, g2);
        box_box_quad(cs, A, B, geom_half(gx, g1), geom_half(gx, g2), poly, poly + 8);
      }
    }
    SYNC();
    PROBE(5, stats, STAT_T_AUX1);
  }
  if (which & 2) {
    for (int k = 0; k < n2; k++) {  // GJK / EPA
      int p, g1, g2;
      cand_unpack(cand[n0 + n1 + k], p, g1, g2);
      const Geom A = geom_lds(gx, g1), B = geom_lds(gx, g2);
      WaveSink cs(&E, p, !only_ro, g1, g2);
      convex_convex(cs, A, B, scr + SCR_EPA, ac, p);
    }
    SYNC();
    PROBE(5, stats, STAT_T_AUX2);
  }
}

// (5) deterministic order: rank sort of the contacts by their 16-bit pair/order key
DEV void collide_sort(EnvSh& E) {
  float* stats = E.stats;
  CLK_DECL;
  float* scr = scr_of(E);
  const int n = min(E.ncon, MMX_MAXCON);
  float* tmp = scr + COL_WORK;
  int kb = 0, rank = 0;
  if (LANE < n) {  // rank by the order key (the key word, with the geoms, travels with the record)
    kb = con_key(crec(E, LANE));
    const int key = kb & 0xFFFF;
    for (int j = 0; j < n; j++) rank += (con_key(crec(E, j)) & 0xFFFF) < key;
#pragma unroll
    for (int f = 0; f < CL_F; f++) tmp[f * MMX_MAXCON + rank] = con_of(E)[f * MMX_MAXCON + LANE];
  }
  SYNC();
  for (int k = LANE; k < MMX_MAXCON * CL_F; k += WG) con_of(E)[k] = tmp[k];
  if (LANE == 0) E.ncon = n;
  SYNC();
  PROBE(5, stats, STAT_T_AUX3);
}

DEV void collide_wave(EnvSh& E, bool only_ro) {
  collide_prune(E, only_ro);
  collide_pairs(E, only_ro, 3);
  if (!only_ro) collide_sort(E);
}
