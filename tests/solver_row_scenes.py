"""A ladder of constraint-row layouts for the solver tests (tests/test_solver_rows_kat.py): test
infrastructure, independent of both implementations under test.

The kernel stores the constraint rows of a substep in one array whose order decides which loop slice and
which memory (LDS below MMX_LDSEFC = 128 or 192 rows, the env's HBM overflow block above) a row is read
from.  `row_layout` restates that order from the kernel's documentation (the comment above
make_constraints_wave in mmx_step_constraints.inc and the block-pair table kTB0 / kTB1 in mmx_step_lds.inc),
not from its code:

* the single rows first: the finger equality, then one row per joint past its range, padded with zero rows
  to a multiple of 4 (`nsingle`: 4, or 8 from four active limits on);
* then the contacts, 4 basis rows (one group) each, grouped by the pair of dof blocks they touch.  Blocks:
  0 = the arm (bodies link1 .. right_finger), 1 / 2 / 3 = the red / green / blue cube, none = a static
  body.  The ten types in order: (0,-) (0,1) (0,2) (0,3) (1,-) (1,2) (1,3) (2,-) (2,3) (3,-); type 0
  starts at row 0 and holds the single rows before its contacts.  `tbase[t]` is type t's first row,
  `tbase[10]` the total.

The scenes are full states (qpos, qvel, ctrl, warm start) built from the builders of cube_contact_scenes.py
and test_collision_kat.py, chosen so that the union of their layouts reaches the edges of the solver's
loops (test_solver_rows_kat.py::test_ladder_premises lists the classes).
"""
from __future__ import annotations

import json
import os

import numpy as np

import cube_contact_scenes as S
from collision_geometry import RawModel
from test_collision_kat import put_cube, scene_cube_edge_on_table, scene_cube_in_bin_corner, scene_cube_tilted_on_floor

HALF = 0.02
NTYPE = 10
TYPE_BLOCKS = [(0, None), (0, 1), (0, 2), (0, 3), (1, None), (1, 2), (1, 3), (2, None), (2, 3), (3, None)]
_MODEL = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mujoco_manip_amd", "model",
                                     "panda_pickplace.json")))
_BODY = [b["name"] for b in _MODEL["bodies"]]
_ARM = {"link1", "link2", "link3", "link4", "link5", "link6", "link7", "hand", "left_finger", "right_finger"}
_CUBE = {"obj_red": 1, "obj_green": 2, "obj_blue": 3}
JNT_RANGE = np.array([j["range"] for j in _MODEL["joints"][:9]])
ARM_GEOMS = {i for i, c in enumerate(_MODEL["col_geoms"]) if _BODY[_MODEL["geoms"][c]["body"]] in _ARM}
TABLE_GEOM = S.TABLE_GEOM


def geom_block(g):
    """Dof block of collision geom g (the id both implementations report): 0 arm, 1..3 cubes, None static."""
    name = _BODY[_MODEL["geoms"][_MODEL["col_geoms"][g]]["body"]]
    return 0 if name in _ARM else _CUBE.get(name)


def contact_type(g1, g2):
    b = sorted(x for x in {geom_block(g1), geom_block(g2)} if x is not None)
    assert b, (g1, g2)  # a contact between two static bodies does not exist
    return TYPE_BLOCKS.index((b[0], b[1] if len(b) > 1 else None))


def row_layout(e):
    """Row layout of the oracle env's current contacts and joint positions: dict(nsingle, nlimit, count =
    contacts per type, tbase[0..10], total = stored rows, ncon)."""
    q = e.get_state()[0]
    nlimit = int(sum((q[j] < JNT_RANGE[j, 0]) + (q[j] > JNT_RANGE[j, 1]) for j in range(9)))
    nsingle = (1 + nlimit + 3) // 4 * 4
    count = [0] * NTYPE
    for c in e.contacts():
        count[contact_type(int(c["geom"][0]), int(c["geom"][1]))] += 1
    tbase, base = [], 0
    for t in range(NTYPE):
        tbase.append(base)
        base += (nsingle if t == 0 else 0) + 4 * count[t]
    tbase.append(base)
    return dict(nsingle=nsingle, nlimit=nlimit, count=count, tbase=tbase, total=base, ncon=sum(count))


def contact_rows(lay, t):
    """[first, end) of type t's contact rows (type 0: behind its single rows)."""
    return lay["tbase"][t] + (lay["nsingle"] if t == 0 else 0), lay["tbase"][t + 1]


# --------------------------------------------------------------------------- building blocks
_CACHE = {}


HELD_STEPS = range(30, 49)


def _held(k, step=40):
    """The oracle expert's state with cube k held in the air, `step` env steps into task (k, k) from the
    keyframe (cube_contact_scenes.held_states is step 40): the carry to the bin.  The finger-cube contact
    set changes from step to step (24 to 34 contacts), which is what moves the later types' bases.  The
    scenes with the red or the blue cube held take other steps than 40: at step 40 their shallowest
    finger-cube contact is 4 and 8 micrometres deep, within 1e-5 m of the contact threshold, where one
    rounding decides whether the contact exists (test_ladder_premises asserts the distance)."""
    import oracle_py as O

    if ("held", k) not in _CACHE:
        e = O.OracleEnv()
        e.reset_keyframe()
        e.fsm_init([(k, k)])
        out = {}
        for n in range(1, HELD_STEPS[-1] + 1):
            e.fsm_plan(16)
            e.fsm_actuate()
            for _ in range(16):
                e.mj_step()
            if n in HELD_STEPS:
                out[n] = e.get_state()
                assert out[n][0][11 + 7 * k] > 0.35
        _CACHE[("held", k)] = out
    return _CACHE[("held", k)][step]


def _raw():
    if "raw" not in _CACHE:
        _CACHE["raw"] = RawModel()
    return _CACHE["raw"]


# the red bin's front-left corner pose of test_collision_kat.scene_cube_in_bin_corner: inner faces
# x = -0.358, y = 0.492, z = 0.242, depths 0.7 / 0.4 / 1.1 mm
CORNER = np.array([-0.358 + HALF - 0.0007, 0.492 + HALF - 0.0004, 0.242 + HALF - 0.0011])
BIN_DX = 0.3  # the green and blue bins sit 0.3 and 0.6 m further along x


def corner_pos(bin_=0, level=0):
    """Centre of a cube in bin `bin_`'s front-left corner; level 1: stacked 0.4 mm deep on the one below."""
    return CORNER + np.array([BIN_DX * bin_, 0.0, level * (2 * HALF - 0.0004)])


def wall_pos(bin_=0):
    """Centre of a cube in bin `bin_` against the left wall and on the bottom only (two faces, 8 contacts)."""
    return CORNER + np.array([BIN_DX * bin_, 0.058 - HALF + 0.0004, 0.0])


def held_scene(k, j, third=None, step=40):
    """Cube k held in the air with cube j pressed under it (cube_contact_scenes.held_on_cube_state); the
    third cube at position `third`, at rest (None: it stays on the table)."""
    q, v, c, w = S.held_on_cube_state({k: _held(k, step)}, k, j)
    if third is not None:
        o = 3 - k - j
        S.put(q, o, third)
        v[9 + 6 * o: 15 + 6 * o] = 0.0
    return q, v, c, w


def held_only(k, places, step=40):
    """Cube k held in the air (the carry state), the other cubes put at `places` = {cube: (pos, R)}, at rest."""
    q, v, c, w = (a.copy() for a in _held(k, step))
    for o, (pos, R) in places.items():
        S.put(q, o, pos, R)
        v[9 + 6 * o: 15 + 6 * o] = 0.0
    return q, v, c, w


def past_limits(state, joints):
    """`state` with the given joints (index, value) moved past their ranges: one limit row each."""
    q, v, c, w = (np.array(a, float) for a in state)
    for j, val in joints:
        assert val < JNT_RANGE[j, 0] or val > JNT_RANGE[j, 1], (j, val)
        q[j] = val
    return q, v, c, w


def kat_scene(f, extra=None):
    """A scene of test_collision_kat.py (the arm at the keyframe, the cubes not named parked in the air)
    as a full state; extra = {cube: (pos, R)} puts further cubes."""
    q = np.array(f(_raw())[0], float)
    for o, (pos, R) in (extra or {}).items():
        put_cube(q, o, pos, R)
    _, v, c, w = S.keyframe_state()
    return q, v, c, w


TIP_TILT = ((4, 0.12), (5, 0.12))  # joint5 and joint6 turned after the IK: the hand leans about both horizontal axes


def fingertips_on_table(depth=0.0005, cubes=None):
    """The hand lowered by the oracle's own IK (gripper open) until a fingertip presses `depth` into the
    tabletop beside the cubes: arm-static contacts, row type 0 with contacts.  The hand leans (TIP_TILT), so
    a fingertip's hull meets the table at a corner: held vertical, its flat end lies face to face on the
    table, where the contact point of two hulls is not unique.  The fingers are 5 mm inside their range: the
    keyframe has them at its upper end to the ulp while the actuator pushes them open, so a one-ulp
    perturbation switches a limit row on or off and the finger's acceleration jumps by 13 m/s^2."""
    key = ("tips", depth)
    if key not in _CACHE:
        q, v, c, w = S.keyframe_state()
        e = S.oracle_env((q, v, c, w))
        xy = np.array([0.075, 0.33])  # 12 cm in front of the cubes' row: the open, leaning fingers stay clear of them

        def pose(z):
            qq = q.copy()
            qq[7:9] = 0.035
            for _ in range(30):  # the IK is one damped step per call: iterate to its fixed point
                e.set_state(qq, v, c, w)
                e.mj_forward()
                qq[:7] = e.ik(np.array([xy[0], xy[1], z]))
            for j, dq in TIP_TILT:
                qq[j] += dq
            e.set_state(qq, v, c, w)
            e.mj_forward()
            tips = [cc for cc in e.contacts() if {int(cc["geom"][0]), int(cc["geom"][1])} & ARM_GEOMS
                    and TABLE_GEOM in (int(cc["geom"][0]), int(cc["geom"][1]))]
            return qq, tips

        lo, hi = 0.30, 0.45  # hand heights: touching at lo, free at hi
        assert pose(lo)[1] and not pose(hi)[1]
        for _ in range(40):  # the height at which the deepest fingertip contact is `depth` deep
            mid = 0.5 * (lo + hi)
            tips = pose(mid)[1]
            if tips and min(cc["dist"] for cc in tips) < -depth:
                lo = mid
            else:
                hi = mid
        _CACHE[key] = pose(lo)[0]
    q, v, c, w = S.keyframe_state()
    q[:9] = _CACHE[key][:9]
    for o, (pos, R) in (cubes or {}).items():
        S.put(q, o, pos, R)
    return q, v, c, w


def finger_touch(k=S.GREEN, j=S.RED, depth=0.0005):
    """Cube k held (the carry state) and cube j pressed `depth` into the outer side of the left finger, in
    the finger's frame: contacts of the arm with two cubes at once (two arm-cube row types).  0.0235 m is
    the clearance at which the cube's face first meets the finger's hull, measured on the oracle."""
    q, v, c, w = (a.copy() for a in _held(k))
    e = S.oracle_env((q, v, c, w))
    p, R = e.body(10)  # left_finger
    S.put(q, j, p + R @ np.array([0.0, 0.0235 - depth + HALF, 0.0445]), R)
    v[9 + 6 * j: 15 + 6 * j] = 0.0
    return q, v, c, w


LIMITS_A = [(7, 0.0402), (8, 0.0402), (6, 2.9), (0, 2.9)]    # both fingers, joint7 and joint1 past the upper end
LIMITS_B = [(7, 0.0402), (8, 0.0402), (6, -2.9), (3, -0.06)]  # joint7 past the lower, joint4 past the upper end


def scenes():
    """[(name, state)] of the ladder, one env per scene (built once)."""
    if "scenes" in _CACHE:
        return _CACHE["scenes"]
    R_, G_, B_ = S.RED, S.GREEN, S.BLUE
    I = np.eye(3)
    out = [
        # a held cube, a second one pressed under it, the third in the red bin's corner (or against one wall)
        ("held:g>r+corner", held_scene(G_, R_, corner_pos(0))),
        ("held:b>r+corner", held_scene(B_, R_, corner_pos(0), step=41)),
        ("held:r>g+corner", held_scene(R_, G_, corner_pos(0), step=47)),
        ("held:r>g+wall", held_scene(R_, G_, wall_pos(0), step=47)),
        ("held:r>g+corner:37", held_scene(R_, G_, corner_pos(0), step=37)),
        ("held:r>g:46", held_scene(R_, G_, None, step=46)),
        ("held:g>b+corner", held_scene(G_, B_, corner_pos(0))),
        # a held cube, the other two in bin corners or stacked in one
        ("held:g+corner_stack", held_only(G_, {R_: (corner_pos(0), I), B_: (corner_pos(0, 1), I)})),
        ("held:b+two_corners", held_only(B_, {R_: (corner_pos(0), I), G_: (corner_pos(1), I)}, step=41)),
        # a held cube and a second cube on a finger's outer side
        ("held:g+finger_touch:r", finger_touch()),
        # piles; with four joints past their ranges nsingle = 8
        ("pile3", S.stack_state(S.CHAINS[1], 0.0004)),
        ("pile3+limits", past_limits(S.stack_state(S.CHAINS[0], 0.0004), LIMITS_A)),
        ("pile2+limits", past_limits(S.stack_state((R_, G_), 0.0004), LIMITS_B)),
        # fingertips on the tabletop beside the resting cubes
        ("fingertips_on_table", fingertips_on_table()),
        # small ones: 1 group, 2 groups, 12 groups
        ("floor_corner", kat_scene(scene_cube_tilted_on_floor)),
        ("table_edge", kat_scene(scene_cube_edge_on_table)),
        ("bin_corner", kat_scene(scene_cube_in_bin_corner)),
    ]
    # the states as the kernel gets them: rounded to fp32
    _CACHE["scenes"] = [(n, tuple(np.asarray(a, np.float32) for a in st)) for n, st in out]
    return _CACHE["scenes"]
