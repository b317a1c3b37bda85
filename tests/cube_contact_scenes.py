"""Scenes and closed forms for the cube-on-cube tests (tests/test_cube_contact_kat.py): test
infrastructure, independent of both implementations under test.

Every scene is a full state (qpos, qvel, ctrl, warm start) built from the keyframe: the arm where
the keyframe has it, cubes not named by a scene resting at their keyframe places (15 cm apart: far
from every stack).  The closed forms extend tests/test_physics_kat.py's (same published equations,
stated in that file's docstring) from one free cube on the static table to two free cubes.
"""
from __future__ import annotations

import json
import os

import numpy as np

from collision_geometry import CUBES, axis_rot, mat2quat, quat2mat
from test_physics_kat import (G, H, HALF, M_CUBE, MU, TABLE_TOP, TRAN, a_hat_pyramid, impedance, kb, make_frame,
                              rest_penetration)

RED, GREEN, BLUE = 0, 1, 2
PAIRS = [(RED, GREEN), (RED, BLUE), (GREEN, BLUE)]                            # (lower, upper): row types 5, 6, 8
CHAINS = [(BLUE, GREEN, RED), (GREEN, RED, BLUE), (RED, BLUE, GREEN)]         # bottom to top: each cube in the middle
HELD = [(k, j) for k in (RED, GREEN, BLUE) for j in (RED, GREEN, BLUE) if j != k]  # (held, placed under it)
KEY_XY = [(-0.15, 0.45), (0.0, 0.45), (0.15, 0.45)]
ROT45 = axis_rot([0, 0, 1], np.pi / 4)

_MODEL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mujoco_manip_amd", "model",
                      "panda_pickplace.json")


def _col_ids():
    cm = json.load(open(_MODEL))
    body = [cm["bodies"][cm["geoms"][c]["body"]]["name"] for c in cm["col_geoms"]]
    kind = [cm["geoms"][c]["type"] for c in cm["col_geoms"]]
    table = next(i for i, (b, t) in enumerate(zip(body, kind)) if b == "table" and t == "box")
    return table, [body.index(n) for n in CUBES]


TABLE_GEOM, CUBE_GEOM = _col_ids()  # ids both implementations report as a contact's geom1 / geom2


def pair_geoms(a, b):
    """The (geom1, geom2) a contact between cubes a and b is reported with: equal types keep the
    lower geom id first."""
    return tuple(sorted((CUBE_GEOM[a], CUBE_GEOM[b])))


# --------------------------------------------------------------------------- closed forms
P_TABLE_1 = rest_penetration(4)                                  # one cube on 4 corners
P_TABLE_2 = rest_penetration(4, load=2 * M_CUBE * G)             # 4 corners under a stack of two: t = 20
P_CUBE = rest_penetration(8, tran=2 * TRAN)                      # 8 octagon corners under one cube: t = 20 + 20
Z_REST_1 = TABLE_TOP + HALF + P_TABLE_1


def stack_rest_heights():
    """Centre heights of a resting two-cube stack (lower, upper)."""
    zl = TABLE_TOP + HALF + P_TABLE_2
    return zl, zl + 2 * HALF + P_CUBE


def first_step_velocity_2(com, rot, v12, table_cons, cube_cons, couple=True):
    """Exact qvel (12) after one substep of two free cubes, the lower one on the static table and
    the upper one on it: the primal problem over 12 dof with every pyramid edge active (checked).
    com, rot: the two centres and rotation matrices (lower, upper); v12 = per cube (linear world,
    angular body); table_cons = [(pos, normal table -> lower, dist)], cube_cons = [(pos, normal
    lower -> upper, dist)].  A cube-cube edge's Jacobian is J_upper - J_lower along that normal,
    its R uses both bodies' invweight (t = 40).  couple=False zeroes the two off-diagonal 6 x 6
    blocks of the system matrix (the block-diagonal solve a missed coupling would do)."""
    K, B = kb()
    I = M_CUBE * (2 * HALF) ** 2 / 6.0
    Mm = np.diag(([M_CUBE] * 3 + [I] * 3) * 2)
    a0 = np.tile([0.0, 0.0, -G, 0.0, 0.0, 0.0], 2)
    A = Mm.copy()
    rhs = Mm @ a0
    rows = []

    def body_J(b, pos, lin, ang):  # 12-vector: the velocity of body b's point at pos along lin, spin about ang
        J = np.zeros(12)
        r = np.asarray(pos, float) - com[b]
        J[6 * b: 6 * b + 3] = lin
        J[6 * b + 3: 6 * b + 6] = rot[b].T @ (np.cross(r, lin) + ang)  # angular velocity in the body frame
        return J

    for cons, tran, bodies in ((table_cons, TRAN, ((0, 1.0),)), (cube_cons, 2 * TRAN, ((1, 1.0), (0, -1.0)))):
        for pos, n, dist in cons:
            F = make_frame(n)
            z3 = np.zeros(3)
            Jn = sum(s * body_J(b, pos, F[0], z3) for b, s in bodies)
            Jk = [sum(s * body_J(b, pos, F[1], z3) for b, s in bodies),
                  sum(s * body_J(b, pos, F[2], z3) for b, s in bodies),
                  sum(s * body_J(b, pos, z3, F[0]) for b, s in bodies)]
            d = impedance(dist)
            D = 1.0 / ((1.0 - d) / d * a_hat_pyramid(tran))
            for k in range(3):
                for sg in (1.0, -1.0):
                    J = Jn + sg * MU[k] * Jk[k]
                    aref = -B * J.dot(v12) - K * d * dist
                    A += D * np.outer(J, J)
                    rhs += D * aref * J
                    rows.append((J, aref))
    if not couple:
        A[:6, 6:] = 0.0
        A[6:, :6] = 0.0
        return v12 + H * np.linalg.solve(A, rhs)
    acc = np.linalg.solve(A, rhs)
    assert all(J.dot(acc) < aref for J, aref in rows), "not every edge active: closed form invalid"
    return v12 + H * acc


def split_contacts(cons, lower, upper):
    """cons = [(g1, g2, dist, pos, normal)]: the table-lower and lower-upper contacts in
    first_step_velocity_2's form (requires lower < upper: the normal then points lower -> upper)."""
    assert lower < upper
    tab = [(np.asarray(c[3], float), np.asarray(c[4], float), float(c[2])) for c in cons
           if (c[0], c[1]) == (TABLE_GEOM, CUBE_GEOM[lower])]
    cc = [(np.asarray(c[3], float), np.asarray(c[4], float), float(c[2])) for c in cons
          if (c[0], c[1]) == (CUBE_GEOM[lower], CUBE_GEOM[upper])]
    return tab, cc


# --------------------------------------------------------------------------- states
def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def keyframe_state():
    """(qpos, qvel, ctrl, warm start) of the keyframe with the three cubes at rest on the table."""
    import oracle_py as O

    e = O.OracleEnv()
    e.reset_keyframe()
    q, v, c, w = e.get_state()
    for o in range(3):
        q[11 + 7 * o] = Z_REST_1
    return q, v, c, w


def put(q, o, pos, R=np.eye(3)):
    q[9 + 7 * o: 12 + 7 * o] = pos
    q[12 + 7 * o: 16 + 7 * o] = mat2quat(R)


def cube(q, o):
    return q[9 + 7 * o: 12 + 7 * o], q[12 + 7 * o: 16 + 7 * o]


def stack_state(order, depth=None):
    """Cubes `order` (bottom to top) stacked at the bottom one's keyframe place, odd levels turned
    45 deg about z.  depth=None: two cubes at the closed-form rest pose; else every level `depth`
    deep in the one below."""
    q, v, c, w = keyframe_state()
    x, y = KEY_XY[order[0]]
    if depth is None:
        assert len(order) == 2
        zs = stack_rest_heights()
    else:
        zs = [TABLE_TOP + HALF - depth + k * (2 * HALF - depth) for k in range(len(order))]
    for lvl, (o, z) in enumerate(zip(order, zs)):
        put(q, o, [x, y, z], ROT45 if lvl % 2 else np.eye(3))
    return q, v, c, w


def held_states():
    """One oracle expert state per cube k with k held in the air: task (k, k) from the keyframe, 40
    env steps on (the carry to the bin, the cube's centre above z = 0.35)."""
    import oracle_py as O

    out = {}
    for k in range(3):
        e = O.OracleEnv()
        e.reset_keyframe()
        e.fsm_init([(k, k)])
        for _ in range(40):
            e.fsm_plan(16)
            e.fsm_actuate()
            for _ in range(16):
                e.mj_step()
        s = e.get_state()
        assert s[0][11 + 7 * k] > 0.35, (k, s[0][11 + 7 * k])
        out[k] = s
    return out


def held_on_cube_state(held, k, j):
    """Cube j put under the held cube k in k's own frame: 0.5 mm into its lower face, turned 45 deg
    about its z, at zero velocity."""
    q, v, c, w = (a.copy() for a in held[k])
    pk, qk = cube(q, k)
    Rk = quat2mat(qk)
    q[9 + 7 * j: 12 + 7 * j] = pk + Rk @ np.array([0.0, 0.0, -(2 * HALF - 0.0005)])
    q[12 + 7 * j: 16 + 7 * j] = _qmul(qk / np.linalg.norm(qk), [np.cos(np.pi / 8), 0.0, 0.0, np.sin(np.pi / 8)])
    v[9 + 6 * j: 15 + 6 * j] = 0.0
    return q, v, c, w


def parity_scenes():
    """[(name, state, cube-cube geom pairs that must touch)]: the coupled states of the GPU-vs-oracle
    parity batch."""
    out = []
    for lo, up in PAIRS:
        out.append((f"stack2:{CUBES[lo]}<{CUBES[up]}", stack_state((lo, up), 0.0004), [pair_geoms(lo, up)]))
    for ch in CHAINS:
        out.append(("stack3:" + "<".join(CUBES[o] for o in ch), stack_state(ch, 0.0004),
                    [pair_geoms(ch[0], ch[1]), pair_geoms(ch[1], ch[2])]))
    held = held_states()
    for k, j in HELD:
        out.append((f"held:{CUBES[k]}>{CUBES[j]}", held_on_cube_state(held, k, j), [pair_geoms(k, j)]))
    return out


def dynamic_scenes():
    """[(name, state, substeps, the two cubes)] of the lockstep scenes."""
    out = []
    q, v, c, w = stack_state((RED, GREEN))
    v[9 + 6 * GREEN] = 0.5
    out.append(("top_push", (q, v, c, w), 40, (RED, GREEN)))
    q, v, c, w = keyframe_state()
    pr, _ = cube(q, RED)
    put(q, GREEN, [pr[0] + 2 * HALF + 0.0005, pr[1], pr[2]])
    v[9 + 6 * RED] = 0.3
    out.append(("side_push", (q, v, c, w), 60, (RED, GREEN)))
    q, v, c, w = keyframe_state()
    pr, _ = cube(q, RED)
    put(q, GREEN, [pr[0] + 0.005, pr[1] + 0.003, pr[2] + 0.060], ROT45)
    out.append(("drop", (q, v, c, w), 150, (RED, GREEN)))
    return out


def oracle_env(state):
    import oracle_py as O

    e = O.OracleEnv()
    e.reset_keyframe()
    e.set_state(*(np.asarray(a, float) for a in state))
    e.mj_forward()
    return e


def oracle_contacts(e):
    return [(int(c["geom"][0]), int(c["geom"][1]), c["dist"], c["pos"], c["frame"][0]) for c in e.contacts()]
