"""Contact forces from the fp64 oracle, in numpy: the reference of the contact-force pass (mmx_contact_forces).
Test infrastructure, independent of the kernel: it reads the oracle's public results only (efc_force, the rows'
types, the contacts with their frames, the body poses, qacc) and the compiled model's friction and condim.

The decode is MuJoCo's documented mj_contactForce / mju_decodePyramid.  The oracle's contact rows are pyramid
edges in contact order, 2 (condim - 1) per contact (1 for condim 1): J_n + mu_k J_k, J_n - mu_k J_k for k = the
two tangents (sliding friction) and, with condim 4, the rotation about the normal (torsional friction).  With
f the edges' forces: fn = sum f, component k = mu_k (f_2k - f_2k+1).  The force acts on geom2's body along the
contact frame (normal from geom1 to geom2), its opposite on geom1's body.

Run as a script it measures the sensitivities `s` from which tests/test_contact_forces_gpu.py takes its bounds.
"""
from __future__ import annotations

import json
import os

import numpy as np

import cube_contact_scenes as S

_MODEL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mujoco_manip_amd", "model",
                      "panda_pickplace.json")
_CM = json.load(open(_MODEL))
_COL = [_CM["geoms"][c] for c in _CM["col_geoms"]]
GEOM_BODY = np.array([g["body"] for g in _COL])
GEOM_FRICTION = np.array([g["friction"] for g in _COL], float)
GEOM_CONDIM = np.array([g["condim"] for g in _COL])
BODIES = (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18)  # the 13 moving bodies, model order
FINGERS, CUBE_BODIES = (10, 11), (16, 17, 18)
M_CUBE, G = 0.05, 9.81
I_CUBE = M_CUBE * 0.04 ** 2 / 6.0
QUANTITIES = ("force", "body_wrench", "touch", "qacc")


def decode(e):
    """Per-contact (geoms [n, 2], pos [n, 3], force [n, 5] = fn, world force on geom2's body, torsional torque)
    of an OracleEnv after mj_forward."""
    cons = e.contacts()
    rows = np.flatnonzero(e.efc()["type"] == 2)
    f = e.efc_force()[rows]
    geoms = np.zeros((len(cons), 2), int)
    pos, force = np.zeros((len(cons), 3)), np.zeros((len(cons), 5))
    at = 0
    for i, c in enumerate(cons):
        g1, g2 = int(c["geom"][0]), int(c["geom"][1])
        dim = int(max(GEOM_CONDIM[g1], GEOM_CONDIM[g2]))
        fr = np.maximum(GEOM_FRICTION[g1], GEOM_FRICTION[g2])
        mu = [fr[0], fr[0], fr[1]][:dim - 1]
        n = 1 if dim == 1 else 2 * (dim - 1)
        ed = f[at:at + n]
        at += n
        comp = np.zeros(4)
        comp[0] = ed.sum()
        for k, m in enumerate(mu):
            comp[1 + k] = m * (ed[2 * k] - ed[2 * k + 1])
        F = c["frame"]
        geoms[i], pos[i] = (g1, g2), c["pos"]
        force[i, 0] = comp[0]
        force[i, 1:4] = comp[0] * F[0] + comp[1] * F[1] + comp[2] * F[2]
        force[i, 4] = comp[3]
    assert at == len(f), (at, len(f))
    return geoms, pos, force, np.array([c["frame"][0] for c in cons]).reshape(-1, 3)


def reference(e):
    """{geoms, pos, force, body_wrench [13, 6], touch [2], qacc [27], contrib} of an OracleEnv after mj_forward;
    contrib [n, 2, 6] = what each contact adds to its two bodies (geom1's, geom2's) about the world origin."""
    geoms, pos, force, normal = decode(e)
    wrench, touch = np.zeros((len(BODIES), 6)), np.zeros(2)
    contrib = np.zeros((len(geoms), 2, 6))
    for i, (g1, g2) in enumerate(geoms):
        b1, b2 = GEOM_BODY[g1], GEOM_BODY[g2]
        F, tau = force[i, 1:4], force[i, 4] * normal[i]
        for side, (b, sg) in enumerate(((b1, -1.0), (b2, 1.0))):
            contrib[i, side] = np.r_[sg * F, sg * (np.cross(pos[i], F) + tau)]
            if b in BODIES:
                x = e.body(int(b))[0]
                wrench[BODIES.index(b)] += np.r_[sg * F, sg * (np.cross(pos[i] - x, F) + tau)]
        for k, fb in enumerate(FINGERS):
            if (b1 == fb and b2 in CUBE_BODIES) or (b2 == fb and b1 in CUBE_BODIES):
                touch[k] += force[i, 0]
    return dict(geoms=geoms, pos=pos, force=force, body_wrench=wrench, touch=touch, qacc=e.qacc(), contrib=contrib)


def qfrc_smooth_norm(e):
    s = e.smooth()
    return float(np.linalg.norm(s["passive"] + s["actuator"] - s["bias"]))


def cube_residuals(ref, q):
    """Per cube o: |m (qacc_lin - g) - F| and |I R qacc_ang - torque about the centre| (the cube's inertia is
    isotropic, its frame origin its centre of mass; its angular velocity is in the body frame)."""
    from collision_geometry import quat2mat

    out = []
    for o in range(3):
        a = ref["qacc"][9 + 6 * o: 15 + 6 * o]
        w = ref["body_wrench"][BODIES.index(16 + o)]
        R = quat2mat(np.asarray(q[12 + 7 * o: 16 + 7 * o], float) / np.linalg.norm(q[12 + 7 * o: 16 + 7 * o]))
        lin = M_CUBE * (a[:3] + np.array([0.0, 0.0, G])) - w[:3]
        ang = I_CUBE * (R @ a[3:]) - w[3:]
        out.append((float(np.linalg.norm(lin)), float(np.linalg.norm(ang))))
    return out


# --------------------------------------------------------------------------- scenes
def fp32_state(state):
    """The state as the device holds it: every array rounded to fp32 (returned as float64)."""
    return tuple(np.asarray(a, np.float32).astype(float) for a in state)


def move_to_bin_state():
    """One oracle expert state mid move_to_bin (FSM state 5): task (red, red) from the keyframe, three env
    steps after the FSM enters the phase."""
    import oracle_py as O

    e = O.OracleEnv()
    e.reset_keyframe()
    e.fsm_init([(0, 0)])
    inside = 0
    for _ in range(120):
        st = e.fsm_plan(16)
        e.fsm_actuate()
        for _ in range(16):
            e.mj_step()
        inside += st == 5
        if inside == 3:
            return e.get_state()
    raise AssertionError("the expert never reached move_to_bin")


_SCENES = None
_EXACT = {}  # name -> the scene's state before the rounding to fp32 (the closed forms hold there)
HELD_ON = [(0, 1), (1, 2), (2, 0)]


def scenes():
    """[(name, class, fp32 state)], built once: the keyframe at rest, the three two-cube stacks, a held cube per
    colour, a held cube pressed on another, one state mid move_to_bin."""
    global _SCENES
    if _SCENES is None:
        out = [("key", "rest", S.keyframe_state())]
        out += [(f"stack:{lo}<{up}", "stack", S.stack_state((lo, up))) for lo, up in S.PAIRS]
        held = S.held_states()
        out += [(f"held:{k}", "held", held[k]) for k in range(3)]
        out += [(f"held_on:{k}>{j}", "held_on", S.held_on_cube_state(held, k, j)) for k, j in HELD_ON]
        out.append(("move_to_bin", "held", move_to_bin_state()))
        _SCENES = [(n, c, fp32_state(s)) for n, c, s in out]
        _EXACT.update({n: tuple(np.asarray(a, float) for a in s) for n, _, s in out})
    return _SCENES


CLASSES = ("rest", "stack", "held", "held_on")


def oracle_at(state, tol=1e-13, maxiter=200):
    import oracle_py as O

    e = O.OracleEnv()
    e.reset_keyframe()
    e.set_solver(tol, maxiter)
    e.set_state(*(np.asarray(a, float) for a in state))
    e.mj_forward()
    return e


_REFS = {}


def scene_reference(name, exact=False):
    """(reference dict, |qfrc_smooth|) of a scene at the oracle's 1e-13 / 200, computed once and not modified.
    exact: from the scene's fp64 state (where the closed forms hold to fp64 rounding) instead of the fp32 state
    the device is given."""
    if (name, exact) not in _REFS:
        state = next(s for n, _, s in scenes() if n == name)
        e = oracle_at(_EXACT[name] if exact else state)
        _REFS[(name, exact)] = (reference(e), qfrc_smooth_norm(e))
    return _REFS[(name, exact)]


# --------------------------------------------------------------------------- comparing two results
def match_contacts(geoms_a, pos_a, geoms_b, pos_b):
    """For every contact of a: the index of b's nearest contact of the same geom pair not taken yet (-1: none),
    and the distance."""
    idx, dist, taken = [], [], set()
    for g, p in zip(geoms_a, pos_a):
        cand = [j for j in range(len(geoms_b)) if tuple(geoms_b[j]) == tuple(g) and j not in taken]
        if not cand:
            idx.append(-1)
            dist.append(np.inf)
            continue
        d = [np.linalg.norm(pos_b[j] - p) for j in cand]
        j = cand[int(np.argmin(d))]
        taken.add(j)
        idx.append(j)
        dist.append(min(d))
    return np.array(idx, int), np.array(dist)


def differences(ref, got):
    """Largest absolute difference per quantity between a reference and another result (same keys; `got` may be
    the device's).  Contacts are matched by geom pair and nearest position; every reference contact whose fn is
    above 1 % of the scene's largest must find a partner (AssertionError otherwise), the others count only when
    they do."""
    idx, _ = match_contacts(ref["geoms"], ref["pos"], got["geoms"], got["pos"])
    fmax = ref["force"][:, 0].max() if len(ref["force"]) else 0.0
    dforce = 0.0
    for i, j in enumerate(idx):
        if j < 0:
            assert ref["force"][i, 0] <= 0.01 * fmax, f"reference contact {i} {tuple(ref['geoms'][i])} has no partner"
            continue
        dforce = max(dforce, float(np.abs(ref["force"][i] - got["force"][j]).max()))
    return {"force": dforce, "body_wrench": float(np.abs(ref["body_wrench"] - got["body_wrench"]).max()),
            "touch": float(np.abs(ref["touch"] - got["touch"]).max()),
            "qacc": float(np.abs(ref["qacc"] - got["qacc"]).max())}


def measure_s(patterns=16, seed=0):
    """{class: {quantity: s}}: per scene the largest change of each quantity when the oracle evaluates the scene
    from qpos / qvel moved by one fp32 ulp per component (`patterns` random sign patterns), plus the change
    between the oracle at 1e-13 / 200 and at the product's 1e-6 / 30; the class takes its scenes' maximum."""
    rng = np.random.default_rng(seed)
    out = {c: dict.fromkeys(QUANTITIES, 0.0) for c in CLASSES}
    for name, cls, state in scenes():
        ref, _ = scene_reference(name)
        q, v, c, w = state
        worst = dict.fromkeys(QUANTITIES, 0.0)
        for _ in range(patterns):
            sq, sv = rng.choice([-1.0, 1.0], len(q)), rng.choice([-1.0, 1.0], len(v))
            q1 = q + sq * np.spacing(np.abs(q).astype(np.float32)).astype(float)
            v1 = v + sv * np.spacing(np.abs(v).astype(np.float32)).astype(float)
            d = differences(ref, reference(oracle_at((q1, v1, c, w))))
            worst = {k: max(worst[k], d[k]) for k in QUANTITIES}
        loose = differences(ref, reference(oracle_at(state, 1e-6, 30)))
        for k in QUANTITIES:
            out[cls][k] = max(out[cls][k], worst[k] + loose[k])
    return out


if __name__ == "__main__":
    print(json.dumps(measure_s(), indent=1))
