"""Contact forces without a GPU: the numpy reference (tests/contact_force_ref.py, the yardstick of the GPU tests)
against closed forms the project already derives, and the two entry points at the C-ABI boundary.

Bounds.  The oracle solves to a gradient of 1e-13 (1 + |qfrc_smooth|) with |qfrc_smooth| below 1e2 in every scene
here, so a force it reports is within ~1e-11 N of the exact solution of its own problem; FP64_N = 1e-9 N leaves
two orders for the conditioning of the problem and the rounding of the decode's sums (loads of 0.5 to 1 N,
eps 1e-16).  A wrong mu, a swapped tangent or a dropped pyramid edge moves a force by its own size (0.1 N and up).
"""
import os
import re

import numpy as np
import pytest

import contact_force_ref as R
import cube_contact_scenes as S
from test_physics_kat import G, M_CUBE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP64_N = 1e-9
MG = M_CUBE * G
NAMES = ("mmx_contact_forces", "mmx_get_force_buffers")


def _normal_load(ref, g1, g2):
    """Sum over the pair's contacts of the force's component along z on geom2's body."""
    sel = [i for i, g in enumerate(ref["geoms"]) if tuple(g) == (g1, g2)]
    return len(sel), sum(ref["force"][i, 3] for i in sel), sum(ref["force"][i, 0] for i in sel)


# --------------------------------------------------------------------------- the reference against closed forms
def test_settled_cube_carries_its_weight():
    """Each cube of the keyframe at its closed-form rest height: four table contacts, together m g = 0.4905 N,
    a quarter each, no tangential force and no torsion."""
    assert abs(MG - 0.4905) < 1e-12
    ref, _ = R.scene_reference("key", exact=True)
    for o in range(3):
        n, fz, fn = _normal_load(ref, S.TABLE_GEOM, S.CUBE_GEOM[o])
        assert n == 4
        assert abs(fz - MG) < FP64_N and abs(fn - MG) < FP64_N, (o, fz, fn)
    table = [i for i, g in enumerate(ref["geoms"]) if g[0] == S.TABLE_GEOM]
    assert np.abs(ref["force"][table, 0] - MG / 4).max() < FP64_N
    assert np.abs(ref["force"][table][:, [1, 2, 4]]).max() < FP64_N
    for o in range(3):
        w = ref["body_wrench"][R.BODIES.index(16 + o)]
        assert np.abs(w - [0, 0, MG, 0, 0, 0]).max() < FP64_N, (o, w)


@pytest.mark.parametrize("pair", S.PAIRS, ids=[f"{a}<{b}" for a, b in S.PAIRS])
def test_stack_carries_two_weights_below_and_one_between(pair):
    lo, up = pair
    ref, _ = R.scene_reference(f"stack:{lo}<{up}", exact=True)
    n, fz, fn = _normal_load(ref, S.TABLE_GEOM, S.CUBE_GEOM[lo])
    assert n == 4 and abs(fz - 2 * MG) < FP64_N and abs(fn - 2 * MG) < FP64_N, (n, fz, fn)
    g1, g2 = S.pair_geoms(lo, up)
    n, fz, fn = _normal_load(ref, g1, g2)
    assert n == 8 and abs(fn - MG) < FP64_N, (n, fn)
    # the force acts on geom2's body: up on the upper cube when it is geom2, down on the lower one otherwise
    assert abs(fz - (MG if g2 == S.CUBE_GEOM[up] else -MG)) < FP64_N, fz
    assert np.abs(ref["body_wrench"][R.BODIES.index(16 + up)] - [0, 0, MG, 0, 0, 0]).max() < FP64_N
    assert np.abs(ref["body_wrench"][R.BODIES.index(16 + lo)] - [0, 0, MG, 0, 0, 0]).max() < FP64_N  # 2 m g - m g


@pytest.mark.parametrize("name", [n for n, _, _ in R.scenes()])
def test_action_equals_reaction_and_newton_euler(name, margin):
    """Every contact adds opposite wrenches to its two bodies; for every cube m (qacc_lin - g) is the body's
    contact force and I qacc_ang its torque about the centre."""
    ref, _ = R.scene_reference(name)
    assert np.abs(ref["contrib"][:, 0] + ref["contrib"][:, 1]).max() == 0.0
    state = next(s for n, _, s in R.scenes() if n == name)
    res = R.cube_residuals(ref, state[0])
    margin("max_newton_euler_residual", max(max(r) for r in res), FP64_N)
    assert max(max(r) for r in res) < FP64_N, res


@pytest.mark.parametrize("name", [n for n, _, _ in R.scenes()])
def test_scene_is_matchable_and_loaded(name):
    """The oracle alone gives a matchable set (contacts of one geom pair lie apart), and every scene class
    carries what it is there for: torsion rows and finger forces in the grasps, cube-cube contacts on a cube."""
    ref, _ = R.scene_reference(name)
    for i in range(len(ref["geoms"])):
        for j in range(i):
            if tuple(ref["geoms"][i]) == tuple(ref["geoms"][j]):
                assert np.linalg.norm(ref["pos"][i] - ref["pos"][j]) > 1e-4, (name, i, j)
    idx, dist = R.match_contacts(ref["geoms"], ref["pos"], ref["geoms"], ref["pos"])
    assert (idx == np.arange(len(idx))).all() and (dist == 0).all()
    if name.startswith(("held", "move_to_bin")):
        assert (ref["touch"] > 0.1).all(), ref["touch"]
        assert np.abs(ref["force"][:, 4]).max() > 1e-6, "no torsional torque in a grasp"  # (N m; rounding: 1e-17)
    if name.startswith("held_on"):
        k, j = int(name[8]), int(name[10])
        assert any(tuple(g) == S.pair_geoms(k, j) for g in ref["geoms"])


def test_decode_discriminates():
    """The decode does depend on what it is given: with the sliding mu halved the held cube's wrench moves by a
    million times FP64_N (and the Newton-Euler check of that scene fails with it)."""
    ref, _ = R.scene_reference("held:0")
    good = ref["body_wrench"][R.BODIES.index(16)].copy()
    keep = R.GEOM_FRICTION.copy()
    try:
        R.GEOM_FRICTION[:, 0] *= 0.5
        state = next(s for n, _, s in R.scenes() if n == "held:0")
        bad_ref = R.reference(R.oracle_at(state))
    finally:
        R.GEOM_FRICTION[:] = keep
    bad = bad_ref["body_wrench"][R.BODIES.index(16)]
    assert np.abs(bad - good).max() > 1e-3, (bad, good)
    assert max(R.cube_residuals(bad_ref, state[0])[0]) > 1e-3


# --------------------------------------------------------------------------- ABI
def _header(name):
    return open(os.path.join(REPO, "include", name)).read()


def _declared(src):
    return set(re.findall(r"^\s*(?:int|int64_t|void|const char\*|uint32_t)\s+(mmx_\w+)\s*\(", src, re.M))


def test_symbols_declared_exported_and_bound():
    from mujoco_manip_amd import _lib

    api, tuning = _declared(_header("mmx_api.h")), _declared(_header("mmx_tuning.h"))
    L = _lib.load()
    for n in NAMES:
        assert n in api and n not in tuning, n
        assert hasattr(L, n), f"libmmx.so does not export {n}"
        assert n in _lib.EXPORTED
    launch = open(os.path.join(REPO, "mujoco_manip_amd", "csrc", "mmx_launch.h")).read()
    assert launch.count("mmx_launch_contact_force(") == 1, "the launcher is declared once"
    hdr = _header("mmx_api.h")
    assert re.search(r"ACTING ON\s+\*?\s*GEOM2'S BODY", hdr) and "not in a snapshot record" in hdr


def test_null_arguments_are_refused():
    from mujoco_manip_amd import _lib

    L = _lib.load()
    assert L.mmx_contact_forces(None) == -1
    b = _lib.MMXForceBuffers()
    assert L.mmx_get_force_buffers(None, b) == -1
    assert not any(getattr(b, n) for n, _ in _lib.MMXForceBuffers._fields_)


def test_force_buffers_match_the_header():
    """MMXForceBuffers is the header's mmx_force_buffers member for member, and the binding's shapes are the
    shapes the header documents."""
    from mujoco_manip_amd import _lib

    hdr = _header("mmx_api.h")
    body = re.search(r"typedef struct \{([^}]*)\} mmx_force_buffers;", hdr).group(1)
    members = re.findall(r"^\s*(int32_t|float\*)\s+(\w+);", body, re.M)
    ctype = {"int32_t": _lib.C.c_int32, "float*": _lib.C.c_void_p}
    assert [(n, ctype[t]) for t, n in members] == list(_lib.MMXForceBuffers._fields_)
    rows = dict(re.findall(r"^ \*     (\w+)\s+((?:\[\w+\])+) fp32", hdr, re.M))
    want = {"contact": f"[N][{_lib.MAXCON}][{_lib.CON_F}]", "force": f"[N][{_lib.MAXCON}][{_lib.FORCE_F}]",
            "body_wrench": f"[N][{len(_lib.FORCE_BODIES)}][6]", "touch": "[N][2]", "qacc": f"[N][{_lib.NV}]",
            "solve": f"[N][{_lib.FORCE_SOLVE_F}]"}
    assert {k: rows.get(k) for k in want} == want
    assert _lib.FORCE_BODIES == R.BODIES and len(_lib.FORCE_SOLVE_FIELDS) == _lib.FORCE_SOLVE_F
    state = open(os.path.join(REPO, "mujoco_manip_amd", "csrc", "mmx_state.h")).read()
    assert f"FRC_F = {_lib.FORCE_F}, FRC_NBODY = {len(_lib.FORCE_BODIES)}, FRC_SOLVE_F = {_lib.FORCE_SOLVE_F}" in state
