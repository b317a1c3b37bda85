"""Narrowphase sweep: every pair class of the compiled model's pair list against exact geometry,
at depth rungs from 50 um to 2.2 cm and at near misses 50 um apart, on the fp64 oracle (CPU) and on
the HIP kernel (`-m gpu`, both step layouts).

Scenes: tests/golden/narrowphase_sweep.json (make_narrowphase_sweep.py; the states are stored as
fp32 values, so the oracle, the kernel and the exact reference all see the same state).  Answers
are derived here from tests/collision_geometry.py: support functions h(n), the overlap along a
direction w(n) = h_1(n) + h_2(-n), the exact depth min_n w(n) (qhull on the Minkowski difference)
and the 15-axis SAT of two boxes.

Checks per scene, on a contact list [(geom1, geom2, dist, pos, normal)]:
  1 pair set: the pairs reported are exactly the pairs whose exact depth is > 0, lower type first;
    a GJK pair gives one contact;
  2 depth is the overlap along the reported normal: |-dist - w(n_rep)| <= tol_depth;
  3 optimality (GJK): 0 <= w(n_rep) - depth_exact <= tol_depth (needs no unique normal);
  4 normal (where the scene's filter allows): angle to the exact normal <= tol_normal;
  5 witnesses: pos - n dist / 2 lies on geom1's surface and pos + n dist / 2 on geom2's (dist < 0:
    geom1 reaches depth / 2 past pos along n, geom2 depth / 2 short of it), within tol_pos;
  6 box-box: the normal is the SAT axis the rule asks for (edge iff edge < 0.95 face), every point
    passes 5, the deepest point is no deeper than the axis overlap, and as deep when the incident
    box's deepest corner projects into the reference face; an edge contact is one point, at the midpoint
    of the two edges' closest points;
  7 kernel against oracle: same contact count per pair, depths equal, and (box and floor pairs, whose
    points the clip chooses) points matched one to one;
  8 no overflow bit in env_error, ncon < MAXCON.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np
import pytest

from collision_geometry import (GOLDEN, ExactScenes, RawModel, box_edge_midpoint, box_expected_axis,
                                box_incident_inside, box_sat, geom_frame, geom_group, overlap, point_to_geom_distance,
                                quat2mat)
from test_collision_kat import CPU_TOL, GPU_TOL_BOX, GPU_TOL_CONVEX, compiled_ids, oracle_contacts

sys.path.insert(0, GOLDEN)
import make_narrowphase_sweep as gen  # noqa: E402

SWEEP = json.load(open(os.path.join(GOLDEN, "narrowphase_sweep.json")))
SCENES = SWEEP["scenes"]
CLASSES = gen.classes_with_scenes(SWEEP)
# The oracle's bounds are test_oracle_mesh_scenes': 1e-8 / 1e-6 / 1e-6 for GJK, CPU_TOL otherwise.  The oracle
# collides the compiled model's hulls, the reference the raw assets' (the compiler reads the OBJ files' decimals
# in double, the hull fixture holds the float32 values): per hull the two vertex sets lie within a computed
# distance of each other (Sweep.hull_shift, at most 1.4e-8), a support value moves by no more, and a pair's
# overlap by the sum over its hulls.  check_scene adds exactly that sum for the pair at hand, on the oracle only.
ORACLE_TOL = dict(box=CPU_TOL, plane=CPU_TOL, gjk=dict(depth=1e-8, normal=1e-6, pos=1e-6))
# A scene's other pairs are whatever the arm's state brings, some of them centimetres deep.  The sweep pins
# depths up to its top rung; a pair deeper than 1.2 x that (the rung's own band) only has to be reported.
BEYOND = 1.2 * max(SWEEP["rungs"])
GPU_TOL = dict(box=GPU_TOL_BOX, plane=GPU_TOL_BOX, gjk=GPU_TOL_CONVEX)


class Sweep:
    """The raw model, the exact answers per scene (computed once, shared by every test of the
    module) and the oracle's contacts per scene."""

    def __init__(self):
        self.m = RawModel()
        self.ids = compiled_ids(self.m)
        self.X = ExactScenes(self.m, self.ids)
        self._exact, self._oracle = {}, {}
        self.seconds = 0.0
        # mesh -> Hausdorff distance between the compiled model's hull vertices and the raw asset's (body frame)
        model = os.path.join(os.path.dirname(GOLDEN), "..", "mujoco_manip_amd", "model", "panda_pickplace.json")
        cm = json.load(open(model))
        self.hull_shift = {}
        for g in (cm["geoms"][c] for c in cm["col_geoms"]):
            if g["type"] == "mesh" and g["mesh"] not in self.hull_shift:
                mesh = next(x for x in cm["meshes"] if x["name"] == g["mesh"])
                V = np.asarray(mesh["verts"]) @ quat2mat(g["quat"]).T + np.asarray(g["pos"])
                d = np.sqrt(((V[:, None] - self.m.hulls[g["mesh"]][None]) ** 2).sum(-1))
                self.hull_shift[g["mesh"]] = float(max(d.min(1).max(), d.min(0).max()))

    def q(self, i):
        return np.array(SCENES[i]["qpos"], np.float32).astype(np.float64)

    def exact(self, i):
        if i not in self._exact:
            t = time.time()
            self._exact[i] = self.X.answers(self.q(i))
            self.seconds += time.time() - t
        return self._exact[i]

    def oracle(self, i):
        if i not in self._oracle:
            self._oracle[i] = oracle_contacts(self.q(i))
        return self._oracle[i]


@pytest.fixture(scope="module")
def sweep():
    return Sweep()


def angle(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b))


def filters_of(S, i, ans, pose):
    """(axis_check, normal_check) of a pair: the stored ones for the meant pair, the same rule from
    the exact answer for every other pair of the scene."""
    s = SCENES[i]
    if [S.ids[ans["g1"]], S.ids[ans["g2"]]] == s["meant"]:
        return s["axis_check"], s["normal_check"]
    return gen.filters(S.m, ans, pose)


def check_scene(S, i, contacts, tol, got=None, hull_shift=None):
    """Checks 1-6 of scene i on a contact list; `tol` maps kind -> dict(depth, normal, pos).
    Measured maxima go into `got` (key -> max).  `hull_shift` (the oracle only): mesh -> how far the
    hull that produced the contacts lies from the reference's; a pair's sum `s` of these is allowed on
    top of the depth and position bounds, and the measured values are recorded less that sum."""
    m, ids, sc = S.m, S.ids, SCENES[i]
    label = f"scene {i} ({sc['cls']}, {sc['kind']} at {sc['rung']:g})"
    got = {} if got is None else got

    def rec(key, v):
        got[key] = max(got.get(key, 0.0), float(v))

    pose = m.fk(S.q(i))
    exact = S.exact(i)
    want = {(ids[a["g1"]], ids[a["g2"]]): a for a in exact if a["depth"] > 0}
    seen = {(c[0], c[1]) for c in contacts}
    swapped = {p for p in seen if (p[1], p[0]) in want and p not in want}
    assert not swapped, f"{label}: pair {swapped} reported in the wrong order (geom1 has the lower type)"
    assert not (set(want) - seen), f"{label}: penetrating pairs not reported: {sorted(set(want) - seen)}"
    assert not (seen - set(want)), f"{label}: contacts on pairs that do not penetrate: {sorted(seen - set(want))}"
    for pair, a in want.items():
        mine = [c for c in contacts if (c[0], c[1]) == pair]
        g1, g2 = m.geoms[a["g1"]], m.geoms[a["g2"]]
        kind = a["kind"]
        t = tol[kind]
        s = sum(hull_shift[g["mesh"]] for g in (g1, g2) if g["type"] == "mesh") if hull_shift else 0.0
        lab = f"{label} pair {pair} {geom_group(g1)}-{geom_group(g2)}"
        axis_ok, normal_ok = filters_of(S, i, a, pose)
        if a["depth"] > BEYOND:
            continue  # deeper than the sweep pins: reported (check 1), and that is all that is asked
        for c in mine:  # 5: witnesses, every point of every kind
            n = np.asarray(c[4], float)
            assert abs(np.linalg.norm(n) - 1) < 10 * t["normal"], f"{lab}: normal not a unit vector"
            for g, p in ((g1, c[3] - n * c[2] / 2), (g2, c[3] + n * c[2] / 2)):
                dsurf = point_to_geom_distance(m, p, g, pose)
                rec(f"{kind}_witness", max(0.0, dsurf - s))
                assert dsurf <= t["pos"] + s, f"{lab}: witness {dsurf:.3g} off the surface of {g['type']}"
        if kind == "plane":
            nz = np.array([0.0, 0.0, 1.0])
            z = np.sort(m.geom_points(g2, pose)[:, 2]) if g2["type"] == "box" else None
            count = min(4, int((z < 0).sum())) if z is not None else 1
            assert len(mine) == count, f"{lab}: {len(mine)} contacts, want {count}"
            for c in mine:
                rec("plane_normal", angle(c[4], nz))
                assert angle(c[4], nz) <= t["normal"], f"{lab}: normal {c[4]}"
            deepest = max(-c[2] for c in mine)
            rec("plane_depth", max(0.0, abs(deepest - a["depth"]) - s))
            assert abs(deepest - a["depth"]) <= t["depth"] + s, f"{lab}: depth {deepest} want {a['depth']}"
            if z is not None:  # the corners below the floor, deepest first
                ds = np.sort([-c[2] for c in mine])[::-1]
                rec("plane_depth", np.abs(ds + z[:count]).max())
                assert np.abs(ds + z[:count]).max() <= t["depth"], f"{lab}: corner depths {ds} want {-z[:count]}"
        elif kind == "gjk":
            assert len(mine) == 1, f"{lab}: {len(mine)} contacts for a convex pair"
            c = mine[0]
            n = np.asarray(c[4], float) / np.linalg.norm(c[4])
            w = overlap(m, g1, g2, pose, n)
            rec("gjk_depth", max(0.0, abs(-c[2] - w) - s))
            assert abs(-c[2] - w) <= t["depth"] + s, f"{lab}: depth {-c[2]} but the overlap along its normal is {w}"
            # on the other hulls the reported normal's overlap is up to s larger and the minimum up to s smaller
            rec("gjk_optimality", max(0.0, w - a["depth"] - 2 * s))
            assert -1e-8 <= w - a["depth"] <= t["depth"] + 2 * s, \
                f"{lab}: overlap along the normal {w}, exact depth {a['depth']}"
            if normal_ok and "cylinder" not in (g1["type"], g2["type"]):
                rec("gjk_normal", angle(n, a["n"]))
                assert angle(n, a["n"]) <= t["normal"], f"{lab}: normal {n} want {a['n']}"
        else:
            check_box(m, lab, mine, a, g1, g2, pose, t, axis_ok, rec)
    return got


def check_box(m, lab, mine, a, g1, g2, pose, t, axis_ok, rec):
    (p1, R1), (p2, R2) = geom_frame(g1, pose), geom_frame(g2, pose)
    face, face_n, edge, edge_n, _ = box_sat(p1, R1, g1["size"], p2, R2, g2["size"])
    n = np.asarray(mine[0][4], float)
    assert all(np.array_equal(c[4], mine[0][4]) for c in mine), f"{lab}: one pair, several normals"
    deepest = max(-c[2] for c in mine)
    # whatever the axis: no point deeper than the overlap along the reported normal
    w = overlap(m, g1, g2, pose, n / np.linalg.norm(n))
    rec("box_depth_over", max(0.0, deepest - w))
    assert deepest <= w + t["depth"], f"{lab}: depth {deepest} exceeds the overlap {w} along its normal"
    if not axis_ok:
        return
    which = box_expected_axis(face, edge)
    ax, ov = (edge_n, edge) if which == "edge" else (face_n, face)
    rec("box_axis", angle(n, ax))
    assert angle(n, ax) <= t["normal"], f"{lab}: normal {n}, want the {which} axis {ax} (face {face}, edge {edge})"
    if which == "edge":
        assert len(mine) == 1, f"{lab}: {len(mine)} contacts for an edge-edge contact"
        rec("box_depth", abs(deepest - ov))
        assert abs(deepest - ov) <= t["depth"], f"{lab}: edge depth {deepest} want {ov}"
        off = np.abs(mine[0][3] - box_edge_midpoint(p1, R1, g1["size"], p2, R2, g2["size"])).max()
        rec("box_edge_pos", off)
        assert off <= t["pos"], f"{lab}: edge contact {off:.3g} off the midpoint of the edges' closest points"
        return
    # face contact: as deep as the overlap when the incident box's deepest corner projects into the reference face
    if box_incident_inside(m, g1, g2, pose)[2]:
        rec("box_depth", abs(deepest - ov))
        assert abs(deepest - ov) <= t["depth"], f"{lab}: deepest point {deepest}, want the face overlap {ov}"


def check_against(S, i, dev, ref, tol):
    """Check 7: the kernel's contacts against the oracle's, pair by pair and point by point."""
    label = f"scene {i} ({SCENES[i]['cls']})"
    kinds = {(S.ids[a["g1"]], S.ids[a["g2"]]): a["kind"] for a in S.exact(i)}
    deep = {(S.ids[a["g1"]], S.ids[a["g2"]]): a["depth"] > BEYOND for a in S.exact(i)}
    out = dict(pos=0.0, depth=0.0, gjk_depth=0.0)
    for pair in sorted({(c[0], c[1]) for c in ref}):
        t = tol[kinds[pair]]
        a = [c for c in dev if (c[0], c[1]) == pair]
        b = [c for c in ref if (c[0], c[1]) == pair]
        assert len(a) == len(b), f"{label} pair {pair}: {len(a)} contacts, the oracle has {len(b)}"
        if deep[pair]:
            continue
        if kinds[pair] == "gjk":  # one contact, its depth unique; its position is not on a face-face contact
            out["gjk_depth"] = max(out["gjk_depth"], abs(a[0][2] - b[0][2]))
            assert abs(a[0][2] - b[0][2]) <= t["depth"], f"{label} pair {pair}: depth {a[0][2]} vs {b[0][2]}"
            continue
        free = list(range(len(b)))
        for c in a:
            d = [np.abs(np.asarray(c[3]) - np.asarray(b[j][3])).max() for j in free]
            j = free.pop(int(np.argmin(d)))
            out["pos"] = max(out["pos"], min(d))
            out["depth"] = max(out["depth"], abs(c[2] - b[j][2]))
            assert min(d) <= t["pos"], f"{label} pair {pair}: no oracle point at {c[3]}"
            assert abs(c[2] - b[j][2]) <= t["depth"], f"{label} pair {pair}: depth {c[2]} vs {b[j][2]}"
    return out


def bound_of(tol, key):
    """The bound a recorded maximum was asserted against: key = <kind>_<what>."""
    kind, what = key.split("_")[:2]
    return tol[kind][{"witness": "pos", "edge": "pos", "normal": "normal", "axis": "normal"}.get(what, "depth")]


def of_class(cls):
    return [i for i, s in enumerate(SCENES) if s["cls"] == cls]


# --------------------------------------------------------------------------- CPU
def test_fixture_regenerates_byte_for_byte():
    """The generator is deterministic.  This is a sample, sized to the CPU suite's time: a cube class
    in full (random poses, parallel edges, overhangs), an arm class in full, and the constructed pad
    scenes of a third are regenerated and compared with the committed lines; the other classes go
    through the same code with other seeds.  The file is the serialiser's output.  The deepest
    expert contact is measured again only by the generator's main()."""
    def lines(scenes):
        return [json.dumps(s, separators=(",", ":")) for s in scenes]

    for cls in ("cube_bin", "plane_pad"):
        assert lines(gen.run(cls)) == lines(s for s in SCENES if s["cls"] == cls), cls
    assert lines(gen.extras("pad_bin")) == lines(s for s in SCENES if s["cls"] == "pad_bin" and "extra" in s)
    assert gen.dump(dict(SWEEP)) == open(os.path.join(GOLDEN, "narrowphase_sweep.json")).read()


def test_census(sweep):
    """Every (type, type, body group) class of the model's pair list has at least 6 scenes per rung
    and 6 near misses, the cube pairs 32 per rung; no filter leaves out more than 5 % of a class; the
    constructed box-box scenes are there and are what their names say.  The one class without scenes
    is listed as uncovered, and geometry says why."""
    m = sweep.m
    model = {gen.class_of(m, a, b) for a, b in sweep.X.pairs}
    assert model == set(SWEEP["classes"]), (model ^ set(SWEEP["classes"]))
    assert SWEEP["uncovered"] == ["pad_pad"] and not any(s["cls"] == "pad_pad" for s in SCENES)
    # the two fingers slide towards each other; shut (both joints at their lower limit) the pads at most touch
    closed = m.fk(gen.f32(gen.parked(m, np.r_[m.key_qpos[:7], 0.0, 0.0])))
    pads = [(a, b) for a, b in sweep.X.pairs if gen.class_of(m, a, b) == "pad_pad"]
    assert pads and all(sweep.X.pair(a, b, closed)["depth"] < 1e-9 for a, b in pads)
    for cls in CLASSES:
        mine = [s for s in SCENES if s["cls"] == cls and "extra" not in s]
        back = {c: r for r, c in sweep.ids.items()}
        for s in mine:
            assert gen.class_of(m, back[s["meant"][0]], back[s["meant"][1]]) == cls
        per = gen.CUBE_PAIR_PER_RUNG if cls == "cube_cube" else gen.PER_RUNG
        for rung in gen.RUNGS:
            assert sum(1 for s in mine if s["kind"] == "hit" and s["rung"] == rung) >= per, (cls, rung)
        # the rung at twice the deepest contact of the expert episodes: everywhere but in three classes of
        # the fingertip pads (4 to 8 mm thick, inside the fingertip hull), where the search finds no state
        if cls not in ("pad_bin", "pad_table", "cube_pad"):
            assert cls not in SWEEP["top_rung_missing"]
            assert sum(1 for s in mine if s["rung"] == gen.TOP_RUNG) >= gen.PER_RUNG, cls
        assert sum(1 for s in mine if s["kind"] == "miss") >= gen.PER_RUNG, cls
        every = [s for s in SCENES if s["cls"] == cls]
        for key in ("axis_check", "normal_check"):
            if key == "normal_check" and cls in gen.CURVED:
                continue
            assert sum(1 for s in every if not s[key]) <= 0.05 * len(every), (cls, key)
    ladder = {f"parallel:{ax}:{ang:g}" for ax in ("face", "diagonal") for ang in (0.0, 3e-7, 1e-5, 1e-3, 1e-2)}
    back = {c: r for r, c in sweep.ids.items()}
    for cls, more in (("cube_cube", "overhang"), ("cube_table", "overhang"), ("cube_bin", "overhang"),
                      ("pad_table", "inside"), ("pad_bin", "inside")):
        extras = {s["extra"]: s for s in SCENES if s["cls"] == cls and "extra" in s}
        assert ladder <= set(extras) and any(k.startswith(more) for k in extras), (cls, sorted(extras))
        for k, s in extras.items():
            if not k.startswith(more):
                continue
            pose = m.fk(np.array(s["qpos"], np.float32).astype(np.float64))
            g1, g2 = (m.geoms[back[c]] for c in s["meant"])
            face, _, edge, _, _ = box_sat(*geom_frame(g1, pose), g1["size"], *geom_frame(g2, pose), g2["size"])
            _, _, inside, over = box_incident_inside(m, g1, g2, pose)
            assert box_expected_axis(face, edge) == "face" and s["axis_check"], (cls, k)
            if more == "overhang":  # the deepest incident corner past the reference face's rim: the clipped case
                assert over > 1e-4, (cls, k, over)
            else:  # the pad, the incident box, inside the large face with every corner of its touching face
                assert inside and geom_group(g1) == "pad" and face == pytest.approx(1e-3, rel=0.2), (cls, k, over)
    assert 2 * SWEEP["deepest_expert_contact"] <= gen.TOP_RUNG == max(SWEEP["rungs"])
    assert os.path.getsize(os.path.join(GOLDEN, "narrowphase_sweep.json")) < 300_000


@pytest.mark.parametrize("cls", CLASSES)
def test_scene_premises_and_oracle(sweep, cls, margin):
    """The fixture's premises from the exact geometry (the meant pair's depth at its rung or its
    gap, every other pair out of the ambiguous band, the stored filters) and the oracle through
    checks 1-6 at fp64 tolerances."""
    got = {}
    for i in of_class(cls):
        s = SCENES[i]
        ans = sweep.exact(i)
        meant = [a for a in ans if [sweep.ids[a["g1"]], sweep.ids[a["g2"]]] == s["meant"]]
        assert len(meant) == 1, i
        d = meant[0]["depth"]
        if s["kind"] == "miss":
            assert -1.8 * gen.GAP <= d <= -0.8 * gen.GAP, (i, d)  # w(n) <= -gap / 2 along the exact normal
        elif "extra" not in s:
            assert 0.8 * s["rung"] <= d <= 1.2 * s["rung"], (i, d)
        for a in ans:
            assert a is meant[0] or a["depth"] > 2e-4, (i, a["g1"], a["g2"], a["depth"])
        assert gen.filters(sweep.m, meant[0], sweep.m.fk(sweep.q(i))) == (s["axis_check"], s["normal_check"]), i
        con = sweep.oracle(i)
        assert len(con) <= 32, (i, len(con))
        check_scene(sweep, i, con, ORACLE_TOL, got, sweep.hull_shift)
    for k, v in got.items():
        margin(k, v, bound_of(ORACLE_TOL, k))
    margin("exact_reference_seconds", round(sweep.seconds, 2))


def _first(pred):
    return next(i for i, s in enumerate(SCENES) if pred(s))


def test_mutations_are_rejected(sweep):
    """The checks at the kernel's tolerances reject: a depth off by 2e-5, a normal turned by 1e-3 rad
    on a polytope pair, a dropped pair, a contact on a near miss, a swapped pair order, and a face
    contact where the edge axis wins clearly.  Base: the oracle's contacts, which pass."""
    S = sweep

    def passes(i, con):
        try:
            check_scene(S, i, con, GPU_TOL)
            return True
        except AssertionError:
            return False

    i = _first(lambda s: s["cls"] == "mesh_mesh" and s["kind"] == "hit" and s["normal_check"] and s["rung"] == 2e-3)
    con = S.oracle(i)
    k = next(j for j, c in enumerate(con) if [c[0], c[1]] == SCENES[i]["meant"])
    assert passes(i, con)
    mut = list(con)
    mut[k] = (con[k][0], con[k][1], con[k][2] - 2e-5, con[k][3], con[k][4])
    assert not passes(i, mut), "a depth off by 2e-5"
    n = np.asarray(con[k][4], float)
    t = np.cross(n, [0.3, 0.5, 0.8])
    n2 = np.cos(1e-3) * n + np.sin(1e-3) * t / np.linalg.norm(t)
    # the turned normal with the depth along it, as a wrong but self-consistent answer would be
    back = {c: r for r, c in S.ids.items()}
    w2 = overlap(S.m, S.m.geoms[back[con[k][0]]], S.m.geoms[back[con[k][1]]], S.m.fk(S.q(i)), n2)
    mut[k] = (con[k][0], con[k][1], -w2, con[k][3], n2)
    assert not passes(i, mut), "a normal turned by 1e-3 rad"
    assert not passes(i, con[:k] + con[k + 1:]), "a dropped pair"
    mut[k] = (con[k][1], con[k][0], con[k][2], con[k][3], -n)
    assert not passes(i, mut), "a swapped pair order"

    i = _first(lambda s: s["cls"] == "cube_hull" and s["kind"] == "miss")
    con = S.oracle(i)
    assert passes(i, con)
    a, b = SCENES[i]["meant"]
    assert not passes(i, con + [(a, b, -1e-6, np.array(SCENES[i]["qpos"][9:12]), np.array([0, 0, 1.0]))]), "a near miss"

    def edge_wins(s):
        if s["cls"] != "cube_cube" or s["kind"] != "hit" or not s["axis_check"] or s["rung"] != 5e-4:
            return False
        q = np.array(s["qpos"], np.float32).astype(np.float64)
        pose = S.m.fk(q)
        g1, g2 = S.m.geoms[back[s["meant"][0]]], S.m.geoms[back[s["meant"][1]]]
        f, _, e, _, _ = box_sat(*geom_frame(g1, pose), g1["size"], *geom_frame(g2, pose), g2["size"])[:5]
        return e < 0.8 * f

    i = _first(edge_wins)
    con = S.oracle(i)
    assert passes(i, con)
    pose = S.m.fk(S.q(i))
    g1, g2 = S.m.geoms[back[con[0][0]]], S.m.geoms[back[con[0][1]]]
    (p1, R1), (p2, R2) = geom_frame(g1, pose), geom_frame(g2, pose)
    face, face_n, *_ = box_sat(p1, R1, g1["size"], p2, R2, g2["size"])
    k = next(j for j, c in enumerate(con) if [c[0], c[1]] == SCENES[i]["meant"])
    mut = [c for j, c in enumerate(con) if j != k] + [(con[k][0], con[k][1], -face, con[k][3], face_n)]
    assert not passes(i, mut), "a face chosen where the edge wins clearly"


# --------------------------------------------------------------------------- GPU
_GPU = {}


def gpu_sweep(rows):
    """All scenes as the envs of one Sim, one substep on the given step layout (run once per layout)."""
    if rows in _GPU:
        return _GPU[rows]
    import torch

    from mujoco_manip_amd import _lib

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    n = len(SCENES)
    t0 = time.time()
    sim = _lib.Sim(n, action_mode="abs_pos", image_size=0)
    sim.reset()
    sim.step_rows = rows
    assert sim.step_rows == rows
    _, _, ctrl, _ = sim.get_state()
    Q = np.array([s["qpos"] for s in SCENES], np.float32)
    sim.set_state(Q, np.zeros((n, 27), np.float32), ctrl, np.zeros((n, 27), np.float32))
    sim.physics_step(1, with_ik=False)
    epi = sim.view("episode_i", _lib.EPI_N, "<i4").cpu().numpy()
    ncon, err = epi[:, _lib.EPI["ncon"]].copy(), epi[:, _lib.EPI["env_error"]].copy()
    con = sim.view("contacts", _lib.MAXCON * _lib.CON_F).cpu().numpy().reshape(n, _lib.MAXCON, _lib.CON_F).copy()
    sim.close()
    lists = [[(int(c[11]), int(c[12]), float(c[0]), c[1:4].astype(float), c[4:7].astype(float)) for c in con[e, :ncon[e]]]
             for e in range(n)]
    _GPU[rows] = dict(lists=lists, ncon=ncon, err=err, raw=con, maxcon=_lib.MAXCON,
                      overflow=_lib.ERR_CON_OVERFLOW | _lib.ERR_EFC_OVERFLOW, seconds=time.time() - t0)
    return _GPU[rows]


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("rows", [128, 192])
def test_gpu_sweep(sweep, rows, cls, margin):
    """Checks 1-8 of one class on one step layout."""
    G = gpu_sweep(rows)
    got, vs = {}, dict(pos=0.0, depth=0.0, gjk_depth=0.0)
    for i in of_class(cls):
        assert G["ncon"][i] < G["maxcon"] and not (G["err"][i] & G["overflow"]), (i, G["ncon"][i], G["err"][i])
        check_scene(sweep, i, G["lists"][i], GPU_TOL, got)
        for k, v in check_against(sweep, i, G["lists"][i], sweep.oracle(i), GPU_TOL).items():
            vs[k] = max(vs[k], v)
    for k, v in got.items():
        margin(k, v, bound_of(GPU_TOL, k))
    margin("oracle_pos", vs["pos"])
    margin("oracle_depth", vs["depth"])
    margin("oracle_gjk_depth", vs["gjk_depth"], GPU_TOL["gjk"]["depth"])
    margin("launch_seconds", round(G["seconds"], 2))


@pytest.mark.gpu
def test_gpu_layouts_give_identical_contact_records():
    """At 192 rows the helper wave runs the GJK pairs while the env wave runs the boxes, both
    reserving contact slots by atomics: the order may differ, the records may not."""
    a, b = gpu_sweep(128), gpu_sweep(192)
    assert np.array_equal(a["ncon"], b["ncon"])
    for e in range(len(SCENES)):
        ra = sorted(r.tobytes() for r in a["raw"][e, :a["ncon"][e]])
        rb = sorted(r.tobytes() for r in b["raw"][e, :b["ncon"][e]])
        assert ra == rb, f"scene {e} ({SCENES[e]['cls']})"
