"""Generates tests/golden/narrowphase_sweep.json: the INPUTS of the narrowphase sweep
(tests/test_narrowphase_sweep.py).  Seeded and deterministic: it regenerates byte for byte.

    python tests/golden/make_narrowphase_sweep.py [--jobs N]

A scene is a state (qpos, stored as the fp32 values both implementations run), the class and rung
it was made for, the pair meant, and the checks it is left out of.  Answers are not stored: the
test derives them from geometry (tests/collision_geometry.py).  The fp64 oracle is used only to
find candidate arm configurations quickly; every scene is accepted by the exact geometry alone:

  * the meant pair's exact depth lies within 20 % of the rung (near misses: 4e-5 .. 9e-5 m apart,
    certified by a separating direction);
  * every other pair of the model's list is certified more than 1e-3 m apart or is more than
    2e-4 m deep;
  * at most 32 contacts can arise (GJK pairs give one, box pairs at most 8, the floor at most 4).

Classes: every (type, type, body group) combination of the model's pair list, see CLASSES.
Arm classes: a uniform arm configuration in which the oracle reports a pair of the class, then a
bisection of one joint on the exact depth.  Cube classes: a cube at a uniformly random orientation
pressed into a random surface point of its partner, then moved out along the exact normal (which
keeps that normal the minimiser) until the depth is the rung.

Constructed box-box scenes (key `extra`, 1 mm deep): `parallel:<axis>:<angle>`, a face-on stack
turned by 0 .. 1e-2 rad about the face axis and a body diagonal (a cube on a cube, the tabletop, a
bin wall; the large finger pad on the tabletop and a bin wall); `overhang:<k>`, the face axis
decides but the deepest incident corner lies past the reference face's rim; `inside`, the pad with
all four corners inside the large face.

Filters, decided here from the exact reference and stored per scene:
  * axis_check = false for a box pair with |edge - 0.95 face| < 2 % of face or two face overlaps
    within 1e-5 of each other whose axes differ (a face-on stack's two faces share one axis);
  * normal_check = false for a polytope GJK pair whose normal_margin is under 5e-5; curved
    (cylinder) pairs never take the normal comparison.
At most 5 % of a class may be left out of a check (asserted); the sampler draws again rather than
take a second filtered scene into a class.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.join(os.path.dirname(TESTS), "oracle"))

from collision_geometry import (ExactScenes, RawModel, axis_rot, box_incident_inside, box_sat, geom_frame,  # noqa: E402
                                geom_group, mat2quat, normal_margin, quat2mat)
from test_collision_kat import compiled_ids  # noqa: E402

RUNGS = [5e-5, 5e-4, 2e-3, 1e-2]
# The deepest contact of the oracle's expert episodes (8 seeds, tasks = all, every physics step:
# measure_deepest below) is 1.09e-2 m, a cube landing on a bin's floor.  Twice that is over the 1e-2
# rung, so there is a rung at 2.2e-2 for every class in which the search finds six such states within
# its budget; the classes where it does not are listed in the fixture (top_rung_missing).
DEEPEST_EXPERT = 0.0109
TOP_RUNG = 2.2e-2
TOP_BUDGET = dict(arm=150000, cube=1500)
GAP = 5e-5
PER_RUNG = 6
CUBE_PAIR_PER_RUNG = 32  # the random cube-pair sweep: 128 poses over the four rungs
RANGES = [(-2.8973, 2.8973), (-1.7628, 1.7628), (-2.8973, 2.8973), (-3.0718, -0.0698), (-2.8973, 2.8973),
          (-0.0175, 3.7525), (-2.8973, 2.8973), (0.0, 0.04), (0.0, 0.04)]
PARK = [[0.8, -0.6, 1.5], [-0.8, -0.6, 1.5], [0.0, -0.9, 1.5]]
# class -> the (group of geom1, group of geom2) combinations it holds; geom1 has the lower type.
# A class with "cube" moves a cube, the others the arm alone.  pad - pad (the two fingers' pads) is
# in the model's pair list but no state inside the joint ranges penetrates it: with both fingers shut
# the small pads just touch (depth 0) and the large ones are 3 mm apart.  It would take a finger past
# its joint limit.  The class is listed as uncovered in the fixture and has no scenes.
CLASSES = {
    "mesh_mesh": [("hull", "hull")], "cyl_mesh": [("leg", "hull")], "cyl_pad": [("leg", "pad")],
    "wall_mesh": [("bin", "hull")], "pad_mesh": [("pad", "hull")], "plane_mesh": [("floor", "hull")],
    "plane_pad": [("floor", "pad")], "pad_bin": [("pad", "bin")], "pad_table": [("pad", "table")],
    "hull_table": [("table", "hull")],
    "cube_cube": [("cube", "cube")], "cube_table": [("table", "cube")], "cube_bin": [("bin", "cube")],
    "cube_leg": [("leg", "cube")], "cube_hull": [("cube", "hull")], "cube_pad": [("pad", "cube")],
    "plane_cube": [("floor", "cube")], "pad_pad": [("pad", "pad")],
}
UNCOVERED = ["pad_pad"]
ARM_CLASSES = [c for c, g in CLASSES.items() if "cube" not in g[0] and c not in UNCOVERED]
CUBE_CLASSES = [c for c, g in CLASSES.items() if "cube" in g[0]]


def class_of(m, a, b):
    ga, gb = geom_group(m.geoms[a]), geom_group(m.geoms[b])
    for c, g in CLASSES.items():
        if (ga, gb) in g or (gb, ga) in g:
            return c
    raise KeyError((ga, gb))


def f32(q):
    return np.asarray(q, np.float32).astype(np.float64)


def short(q):
    """fp32 values in their shortest decimal form: np.float32 of each gives the value back."""
    out = [float(str(np.float32(v))) for v in q]
    assert np.array_equal(np.asarray(out, np.float32), np.asarray(q, np.float32))
    return out


def parked(m, arm):
    q = m.key_qpos.copy()
    q[:9] = arm
    for k in range(3):
        q[9 + 7 * k: 12 + 7 * k] = PARK[k]
        q[12 + 7 * k: 16 + 7 * k] = [1, 0, 0, 0]
    return q


def filters(m, ans, pose):
    """(axis_check, normal_check) of the meant pair's exact answer."""
    if ans["kind"] == "box":
        ga, gb = m.geoms[ans["g1"]], m.geoms[ans["g2"]]
        (pa, Ra), (pb, Rb) = geom_frame(ga, pose), geom_frame(gb, pose)
        face, _, edge, _, faces = box_sat(pa, Ra, ga["size"], pb, Rb, gb["size"])
        # two face overlaps within 1e-5 leave the axis open, unless the two axes are one and the same
        # direction (a face-on stack: within 2e-6 rad, a fifth of the normal tolerance)
        axes = [R[:, k] for R in (Ra, Rb) for k in range(3)]
        k0 = int(np.argmin(faces))
        tie = any(k != k0 and faces[k] - faces[k0] < 1e-5 and abs(axes[k] @ axes[k0]) < np.cos(2e-6) for k in range(6))
        return bool(abs(edge - 0.95 * face) >= 0.02 * face and not tie), True
    if ans["kind"] == "gjk":
        curved = "cylinder" in (m.geoms[ans["g1"]]["type"], m.geoms[ans["g2"]]["type"])
        return True, bool(not curved and normal_margin(ans["facets"]) >= 5e-5)
    return True, True


def accept(X, q, meant, lo, hi):
    """The scene's premises at the fp32 state q: the meant pair's depth in [lo, hi], every other
    pair clear of the ambiguous band, at most 32 contacts.  Returns the meant answer or None."""
    m = X.m
    ans = X.answers(q)
    mine = [a for a in ans if (a["g1"], a["g2"]) == meant]
    if not mine or not lo <= mine[0]["depth"] <= hi:  # a near miss (lo < hi < 0): apart by -hi .. -lo
        return None
    ncon = 0
    for a in ans:
        if (a["g1"], a["g2"]) != meant and a["depth"] <= 2e-4:
            return None  # nearer than 1e-3 and not clearly penetrating
        if not a.get("exact", True):
            return None  # a deep curved pair whose exact depth did not settle
        ncon += {"gjk": 1, "box": 8, "plane": 4 if m.geoms[a["g2"]]["type"] == "box" else 1}[a["kind"]]
    if ncon > 32:
        return None
    if meant[0] == 0 and m.geoms[meant[1]]["type"] == "box":
        # floor - box: which corners lie below the floor must be beyond doubt
        z = m.geom_points(m.geoms[meant[1]], m.fk(q))[:, 2]
        if lo > 0 and np.abs(np.sort(z)[1:]).min() < GAP:
            return None
    return mine[0]


# --------------------------------------------------------------------------- arm classes
def arm_class_scenes(cls):
    import oracle_py as O

    m = RawModel()
    ids = compiled_ids(m)
    back = {c: r for r, c in ids.items()}
    X = ExactScenes(m, ids)
    rng = np.random.default_rng([14, list(CLASSES).index(cls)])
    env = O.OracleEnv()
    env.reset_keyframe()
    want = [(r, "hit") for r in RUNGS for _ in range(PER_RUNG)] + [(RUNGS[1], "miss")] * PER_RUNG
    base = len(want)
    want += [(TOP_RUNG, "hit")] * PER_RUNG
    out, tries = [], 0
    while len(out) < len(want):
        tries += 1
        if len(out) == base and tries > 0:
            base, tries = -1, 0  # the regular scenes are in: the top rung has a budget of its own
        if base == -1 and tries > TOP_BUDGET["arm"]:
            out = [s for s in out if s["rung"] != TOP_RUNG]
            break
        assert tries < 3000000, (cls, len(out))
        arm = np.array([rng.uniform(*r) for r in RANGES])
        arm[8] = arm[7] if rng.uniform() < 0.5 else arm[8]
        q = parked(m, arm)
        env.set_state(q, np.zeros(27), None, np.zeros(27))
        env.mj_forward()
        found = sorted({(back[int(c["geom"][0])], back[int(c["geom"][1])]) for c in env.contacts()})
        found = [p for p in found if class_of(m, *p) == cls]
        if not found:
            continue
        meant = found[rng.integers(len(found))]
        rung, kind = want[len(out)]
        target = rung if kind == "hit" else -1.5 * GAP
        lo, hi = (0.8 * rung, 1.2 * rung) if kind == "hit" else (-1.8 * GAP, -0.8 * GAP)
        j = int(rng.integers(0, 7))

        def depth(s):
            qq = q.copy()
            qq[j] = s
            return X.pair(*meant, m.fk(f32(qq)), nfacets=1)["depth"] - target

        s0, f0 = q[j], depth(q[j])  # bracket the target between the state found and a nearby one
        s1 = None
        for step in (0.02, -0.02, 0.06, -0.06, 0.15, -0.15):
            s = s0 + step
            if RANGES[j][0] < s < RANGES[j][1] and depth(s) * f0 < 0:
                s1 = s
                break
        if s1 is None:
            continue
        if f0 < 0:
            s0, s1 = s1, s0  # s0 is the side deeper than the target
        for _ in range(40):
            mid = 0.5 * (s0 + s1)
            fm = depth(mid)
            if fm > 0:
                s0 = mid
            else:
                s1 = mid
            if lo - target <= fm <= hi - target and abs(fm) < 0.1 * abs(target):
                s0 = s1 = mid
                break
        q[j] = 0.5 * (s0 + s1)
        q = f32(q)
        ans = accept(X, q, meant, lo, hi)
        if ans is None:
            continue
        axis_ok, normal_ok = filters(m, ans, m.fk(q))
        if over_budget(cls, out, axis_ok, normal_ok):
            continue
        out.append(dict(cls=cls, rung=rung, kind=kind, meant=[ids[meant[0]], ids[meant[1]]], axis_check=axis_ok,
                        normal_check=normal_ok, qpos=short(q)))
    return cap_filters(cls, out)


# --------------------------------------------------------------------------- cube classes
def random_rotation(rng):
    q = rng.normal(size=4)
    return quat2mat(q / np.linalg.norm(q))


def surface_point(m, g, pose, rng):
    """A random point on a geom's surface and a direction u pointing out of it there."""
    if g["type"] == "plane":
        return np.array([rng.uniform(0.6, 1.2), rng.uniform(-1.0, -0.3), 0.0]), np.array([0.0, 0.0, 1.0])
    if g["type"] == "mesh":
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        W = m.geom_points(g, pose)
        return W[np.argmax(W @ u)], u
    c, R = geom_frame(g, pose)
    if g["type"] == "cylinder":
        a, z = rng.uniform(0, 2 * np.pi), rng.uniform(-0.9, 0.9) * g["size"][1]
        u = R @ np.array([np.cos(a), np.sin(a), 0.0])
        return c + g["size"][0] * u + R[:, 2] * z, u
    h = np.asarray(g["size"], float)
    area = np.array([h[1] * h[2], h[0] * h[2], h[0] * h[1]])
    k = int(rng.choice(3, p=area / area.sum()))
    s = 1.0 if rng.uniform() < 0.5 else -1.0
    loc = rng.uniform(-1, 1, size=3) * h
    loc[k] = s * h[k]
    return c + R @ loc, s * R[:, k]


def cube_scene(m, X, ids, cls, rung, rng, R=None, partner=None, x_u=None):
    """One attempt at a cube scene of a class; None when the attempt fails a premise."""
    arm = np.r_[m.key_qpos[:7], 0.03, 0.03]
    q = parked(m, arm)
    cube = m.find("obj_red", "box")
    want = [g for g in CLASSES[cls][0] if g != "cube"]
    if cls == "cube_cube":
        other = m.find("obj_green", "box")
        q[16:19] = [rng.uniform(0.5, 0.8), rng.uniform(-0.5, 0.0), rng.uniform(0.5, 1.0)]
        q[19:23] = mat2quat(random_rotation(rng))
    elif partner is not None:
        other = partner
    else:
        cand = [i for i, g in enumerate(m.geoms) if geom_group(g) == want[0]
                and not (cls == "cube_hull" and g["body"] in ("link0", "link1"))]
        other = cand[rng.integers(len(cand))]
    q = f32(q)
    pose = m.fk(q)
    x, u = x_u if x_u is not None else surface_point(m, m.geoms[other], pose, rng)
    R = random_rotation(rng) if R is None else R
    reach = np.abs(R.T @ u) @ np.full(3, 0.02)  # the cube's support along -u
    q[9:12] = x + u * (reach - 1.3 * max(rung, 1e-3))
    q[12:16] = mat2quat(R)
    q = f32(q)
    a, b, _ = X.order(other, cube, u)
    sign = 1.0 if b == cube else -1.0  # the exact normal points g1 -> g2
    first = X.pair(a, b, m.fk(q), nfacets=1)
    if first["depth"] < rung:
        return None
    q[9:12] += sign * first["n"] * (first["depth"] - rung)
    q = f32(q)
    ans = accept(X, q, (a, b), 0.8 * rung, 1.2 * rung)
    if ans is None:
        return None
    axis_ok, normal_ok = filters(m, ans, m.fk(q))
    scene = dict(cls=cls, rung=rung, kind="hit", meant=[ids[a], ids[b]], axis_check=axis_ok, normal_check=normal_ok,
                 qpos=short(q))
    miss = None
    if rung == RUNGS[1]:
        q2 = q.copy()
        q2[9:12] += sign * ans["n"] * (ans["depth"] + 1.5 * GAP)
        q2 = f32(q2)
        if accept(X, q2, (a, b), -1.8 * GAP, -0.8 * GAP) is not None:
            miss = dict(scene, kind="miss", qpos=short(q2))
    return scene, miss


def cube_class_scenes(cls):
    m = RawModel()
    ids = compiled_ids(m)
    X = ExactScenes(m, ids)
    rng = np.random.default_rng([15, list(CLASSES).index(cls)])
    per = CUBE_PAIR_PER_RUNG if cls == "cube_cube" else PER_RUNG
    out = []
    for rung in RUNGS + [TOP_RUNG]:
        got, misses, tries = [], [], 0
        per = PER_RUNG if rung == TOP_RUNG else per
        while len(got) < per:
            tries += 1
            if rung == TOP_RUNG and tries > TOP_BUDGET["cube"]:
                got = []
                break
            assert tries < 20000, (cls, rung)
            res = cube_scene(m, X, ids, cls, rung, rng)
            if res is None or (rung == RUNGS[1] and res[1] is None and len(misses) < PER_RUNG):
                continue
            if over_budget(cls, out + got, res[0]["axis_check"], res[0]["normal_check"]):
                continue
            got.append(res[0])
            if res[1] is not None and len(misses) < PER_RUNG:
                misses.append(res[1])
        out += got + misses
    if cls in ("cube_cube", "cube_table", "cube_bin"):
        out += parallel_edge_scenes(m, X, ids, cls, rng)
    return cap_filters(cls, out)


def parallel_edge_scenes(m, X, ids, cls, rng):
    """A cube face-on on its partner, 1 mm deep, turned by 0, 3e-7, 1e-5, 1e-3 and 1e-2 rad about
    the face axis and about a body diagonal: edges that are parallel or nearly so, where the SAT
    normalises cross products just above its 1e-6 cutoff."""
    out = []
    for axis_name, axis in (("face", None), ("diagonal", np.ones(3) / np.sqrt(3))):
        for ang in (0.0, 3e-7, 1e-5, 1e-3, 1e-2):
            for _ in range(200):
                # the tabletop's upper face; a bin's left wall's inner face (its floor lies 1 mm over the
                # tabletop, which would sit in the band no other pair may be in)
                partner = {"cube_table": m.find("table", "box"), "cube_bin": m.find("bin_green", "box", 3)}.get(cls)
                q = f32(parked(m, np.r_[m.key_qpos[:7], 0.03, 0.03]))
                x_u, base = None, np.eye(3)
                if cls != "cube_cube":
                    c, _ = geom_frame(m.geoms[partner], m.fk(q))
                    h = m.geoms[partner]["size"]
                    if cls == "cube_table":
                        x_u = (c + [rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), h[2]], np.array([0, 0, 1.0]))
                    else:
                        x_u = (c + [h[0], rng.uniform(-0.03, 0.03), rng.uniform(-0.005, 0.005)], np.array([1.0, 0, 0]))
                        base = axis_rot([0, 1, 0], np.pi / 2)  # the cube's z face against the wall
                R = base @ axis_rot([0, 0, 1] if axis is None else axis, ang)
                if cls == "cube_cube":
                    res = stacked_cubes(m, X, ids, R, rng)
                else:
                    res = cube_scene(m, X, ids, cls, 1e-3, rng, R=R, partner=partner, x_u=x_u)
                if res is not None:
                    out.append(dict(res[0], extra=f"parallel:{axis_name}:{ang:g}"))
                    break
            else:
                raise AssertionError((cls, axis_name, ang))
    return out


def stacked_cubes(m, X, ids, Rrel, rng):
    """The red cube face-on on the green one, 1 mm deep, both turned by a common random rotation
    and the upper one by Rrel on top of it."""
    q = parked(m, np.r_[m.key_qpos[:7], 0.03, 0.03])
    R0 = random_rotation(rng)
    c0 = np.array([rng.uniform(0.5, 0.8), rng.uniform(-0.5, 0.0), rng.uniform(0.5, 1.0)])
    q[16:19], q[19:23] = c0, mat2quat(R0)
    off = np.array([rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), 0.04 - 1e-3])
    q[9:12], q[12:16] = c0 + R0 @ off, mat2quat(R0 @ Rrel)
    q = f32(q)
    a, b = m.find("obj_red", "box"), m.find("obj_green", "box")
    ans = accept(X, q, (a, b), 0.5e-3, 1.2e-3)
    if ans is None:
        return None
    axis_ok, normal_ok = filters(m, ans, m.fk(q))
    return dict(cls="cube_cube", rung=1e-3, kind="hit", meant=[ids[a], ids[b]], axis_check=axis_ok,
                normal_check=normal_ok, qpos=short(q)), None


def overhang_scenes(m, X, ids, cls, rng, count=3):
    """Random cube poses 1 mm deep in which the face axis decides (clear of both filters) and the
    cube's deepest corner along it lies more than 1e-4 past the reference face's rim: the clip
    removes that corner, so the deepest contact is shallower than the axis overlap."""
    out = []
    for _ in range(4000):
        res = cube_scene(m, X, ids, cls, 1e-3, rng)
        if res is None or not res[0]["axis_check"]:
            continue
        q = f32(res[0]["qpos"])
        pose = m.fk(q)
        a, b = ({c: r for r, c in ids.items()}[k] for k in res[0]["meant"])
        ga, gb = m.geoms[a], m.geoms[b]
        face, _, edge, _, _ = box_sat(*geom_frame(ga, pose), ga["size"], *geom_frame(gb, pose), gb["size"])
        if edge < 0.95 * face or box_incident_inside(m, ga, gb, pose)[3] < 1e-4:
            continue
        out.append(dict(res[0], extra=f"overhang:{len(out)}"))
        if len(out) == count:
            return out
    raise AssertionError((cls, len(out)))


def arm_to(m, body, local, p_want, R_want):
    """The parked state whose arm joints bring the point `local` of `body` to p_want with the body's
    rotation R_want: least squares from the key pose inside the joint ranges, fingers open.  None
    when the pose is out of reach."""
    from scipy.optimize import least_squares

    q0 = parked(m, np.r_[m.key_qpos[:7], 0.04, 0.04])
    local = np.asarray(local, float)

    def res(arm):
        q = q0.copy()
        q[:7] = arm
        p, R = m.fk(q)[body]
        E = R_want.T @ R
        return np.r_[p + R @ local - p_want, 0.1 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])]

    lo, hi = (np.array(v) for v in zip(*RANGES[:7]))
    sol = least_squares(res, np.clip(m.key_qpos[:7], lo + 1e-3, hi - 1e-3), bounds=(lo, hi), xtol=1e-15, ftol=1e-15,
                        gtol=1e-15)
    if np.abs(sol.fun).max() > 1e-9:
        return None
    q0[:7] = sol.x
    return q0


def pad_scenes(cls):
    """The left finger's large pad (8.5 x 4 x 8.5 mm) face-on and 1 mm deep in a large face, the
    hand upright: its tip face on the tabletop (pad_table), a side face on the inner face of a bin's
    left wall (pad_bin).  `inside`: at a random turn about the face axis, all four corners inside
    the large face.  `parallel`: turned by 0, 3e-7, 1e-5, 1e-3 and 1e-2 rad about the face axis and
    about the pad's diagonal from the pose whose edges are parallel to the large face's.  The arm
    carries the pad, so the turn is the nominal one to within the fp32 rounding of seven joint
    angles, about 2e-7 rad: the two lowest rungs both land at cross products about or below the
    SAT's 1e-6 cutoff, which is what they are for.  The pad sits 15 mm inside the face's rim with
    the other finger, 80 mm away, past the rim, so that only one finger's pads touch."""
    m = RawModel()
    ids = compiled_ids(m)
    X = ExactScenes(m, ids)
    rng = np.random.default_rng([16, list(CLASSES).index(cls)])
    pad = m.find("left_finger", "box")
    g = m.geoms[pad]
    h = np.asarray(g["size"], float)
    rest = f32(parked(m, np.r_[m.key_qpos[:7], 0.04, 0.04]))
    down = np.array([0.0, 0.0, -1.0])
    if cls == "pad_table":
        partner, k = m.find("table", "box"), 2  # the pad's tip face (+z of the finger frame)
    else:
        partner, k = m.find("bin_green", "box", 3), 0
    c, Rp = geom_frame(m.geoms[partner], m.fk(rest))
    hp = np.asarray(m.geoms[partner]["size"], float)
    turns = [("inside", None, None)]
    for name, axis in (("face", np.eye(3)[k]), ("diagonal", np.ones(3) / np.sqrt(3))):
        turns += [(f"parallel:{name}:{ang:g}", axis, ang) for ang in (0.0, 3e-7, 1e-5, 1e-3, 1e-2)]
    out = []
    for tag, axis, ang in turns:
        for _ in range(40):
            s = 1.0 if rng.uniform() < 0.5 else -1.0
            if cls == "pad_table":  # near the rim at x = +- hx or y = +- hy of the top face
                e = int(rng.integers(2))
                t = np.zeros(3)
                t[e], t[1 - e], t[2] = s * (hp[e] - 0.015), rng.uniform(-0.5, 0.5) * hp[1 - e], hp[2]
                u, y = Rp[:, 2], -s * Rp[:, e]  # the finger's y points inward: the other finger lies at -80 mm y
                Rf = np.stack([np.cross(y, down), y, down], axis=1)
            else:  # near the wall's end at y = +- hy, the other finger past it
                t = np.array([hp[0], s * (hp[1] - 0.015), rng.uniform(-0.005, 0.005)])
                u, y = Rp[:, 0], -s * Rp[:, 1]
                Rf = np.stack([np.cross(y, down), y, down], axis=1)  # the finger's x is +- u
            if tag == "inside":
                Rf = Rf @ axis_rot(np.eye(3)[k], rng.uniform(0.1, 0.4))
            else:
                Rf = Rf @ axis_rot(axis, ang)
            reach = np.abs(Rf.T @ u) @ h
            q = arm_to(m, "left_finger", g["pos"], c + Rp @ t + u * (reach - 1e-3), Rf)
            if q is None:
                continue
            q = f32(q)
            a, b, _ = X.order(partner, pad, u)
            ans = accept(X, q, (a, b), 0.5e-3, 1.2e-3)
            if ans is None:
                continue
            pose = m.fk(q)
            if tag == "inside" and not box_incident_inside(m, m.geoms[a], m.geoms[b], pose)[2]:
                continue
            axis_ok, normal_ok = filters(m, ans, pose)
            out.append(dict(cls=cls, rung=1e-3, kind="hit", meant=[ids[a], ids[b]], axis_check=axis_ok,
                            normal_check=normal_ok, qpos=short(q), extra=tag))
            break
        else:
            raise AssertionError((cls, tag))
    return out


CURVED = ("cyl_mesh", "cyl_pad", "cube_leg")  # never take the normal comparison


def over_budget(cls, scenes, axis_ok, normal_ok):
    """Resample rather than exceed the cap: one scene per class and check may be a filtered one."""
    if not axis_ok and any(not s["axis_check"] for s in scenes):
        return True
    return cls not in CURVED and not normal_ok and any(not s["normal_check"] for s in scenes)


def cap_filters(cls, scenes):
    """At most 5 % of a class left out of any one check: the surplus filtered scenes cannot simply be
    kept, so the generator fails loudly and the seed or the sampler is changed."""
    for key in ("axis_check", "normal_check"):
        if cls in CURVED and key == "normal_check":
            continue
        out = sum(1 for s in scenes if not s[key])
        assert out <= 0.05 * len(scenes), (cls, key, out, len(scenes))
    return scenes


def measure_deepest(seeds=8):
    """The deepest contact over the oracle's expert episodes, every physics step (CPU, about 5 s)."""
    import oracle_py as O
    sys.path.insert(0, os.path.dirname(TESTS))
    from mujoco_manip_amd.constants import BINS, OBJECTS, TASK_SETS

    pool = [(OBJECTS.index(o), BINS.index(b)) for o, b in TASK_SETS["all"]]
    worst = 0.0
    for seed in range(seeds):
        e = O.OracleEnv(action_mode="abs_pos", reward_type="staged", randomize_objects=True, tasks=pool)
        e.reset(seed=seed)
        e.fsm_init([e.task()])
        for _ in range(500 * 16):
            if e.fsm_plan(1) == 10:
                break
            e.fsm_actuate()
            e.mj_step()
            worst = max([worst] + [-c["dist"] for c in e.contacts()])
    return worst


OVERHANGS = ("cube_cube", "cube_table", "cube_bin")


def extras(cls):
    """The constructed box-box scenes beyond the parallel-edge ladder of the cube classes, from a
    random stream of their own: overhangs (the cube against a cube, the tabletop, a bin), the pad
    inside a large face and the pad's ladder (pad_table, pad_bin)."""
    if cls in ("pad_table", "pad_bin"):
        return pad_scenes(cls)
    if cls in OVERHANGS:
        m = RawModel()
        ids = compiled_ids(m)
        return overhang_scenes(m, ExactScenes(m, ids), ids, cls, np.random.default_rng([16, list(CLASSES).index(cls)]))
    return []


def run(cls):
    base = arm_class_scenes(cls) if cls in ARM_CLASSES else cube_class_scenes(cls)
    return cap_filters(cls, base + extras(cls))


def generate(jobs=1, classes=None):
    classes = [c for c in CLASSES if c not in UNCOVERED] if classes is None else classes
    if jobs > 1:
        with Pool(jobs) as pool:
            parts = pool.map(run, classes, chunksize=1)
    else:
        parts = [run(c) for c in classes]
    scenes = [s for p in parts for s in p]
    missing = [c for c, p in zip(classes, parts) if not any(s["rung"] == TOP_RUNG for s in p)]
    return dict(_source="tests/golden/make_narrowphase_sweep.py", rungs=RUNGS + [TOP_RUNG], gap=GAP,
                deepest_expert_contact=DEEPEST_EXPERT, top_rung_missing=missing, uncovered=UNCOVERED,
                classes={c: [list(p) for p in g] for c, g in CLASSES.items()}, scenes=scenes)


def classes_with_scenes(doc):
    return [c for c in doc["classes"] if c not in doc["uncovered"]]


def dump(doc):
    head = {k: v for k, v in doc.items() if k != "scenes"}
    lines = [json.dumps(s, separators=(",", ":")) for s in doc["scenes"]]
    return json.dumps(head)[:-1] + ', "scenes": [\n' + ",\n".join(lines) + "\n]}\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--classes", nargs="*")
    ap.add_argument("--out", default=os.path.join(HERE, "narrowphase_sweep.json"))
    a = ap.parse_args()
    deepest = measure_deepest()
    print("deepest expert contact", deepest)
    assert abs(deepest - DEEPEST_EXPERT) < 1e-4 and 2 * DEEPEST_EXPERT <= TOP_RUNG, deepest
    doc = generate(a.jobs, a.classes)
    for c in classes_with_scenes(doc):
        mine = [s for s in doc["scenes"] if s["cls"] == c]
        print(c, len(mine), "axis filtered", sum(not s["axis_check"] for s in mine), "normal filtered",
              sum(not s["normal_check"] for s in mine))
    with open(a.out, "w") as f:
        f.write(dump(doc))


if __name__ == "__main__":
    main()
