"""The trajectory rollout's C-ABI boundary, without a GPU: mmx_rollout_actions and
mmx_rollout_expert_record are declared in include/mmx_api.h (the reference boundary: they stand for the
driver loops of replay_actions.py and generate_dataset.py), exported and bound; the binding's
MMXTrajectory has the header struct's members in the header's order; a NULL sim is refused."""
import ctypes as C
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mmx_rollout_actions", "mmx_rollout_expert_record")


def _header(name="mmx_api.h"):
    return open(os.path.join(REPO, "include", name)).read()


def test_symbols_declared_exported_and_bound():
    from mujoco_manip_amd import _lib

    api, tuning = _header(), _header("mmx_tuning.h")
    L = _lib.load()
    for sym in SYMBOLS:
        assert re.search(rf"^int\s+{sym}\s*\(", api, re.M), f"{sym} not declared in mmx_api.h"
        assert sym not in tuning
        assert hasattr(L, sym), f"libmmx.so does not export {sym}"
        assert sym in _lib.EXPORTED


def test_trajectory_struct_matches_header():
    from mujoco_manip_amd import _lib

    body = re.search(r"typedef struct \{([^}]*)\}\s*mmx_trajectory\s*;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, name = re.fullmatch(r"(float|int32_t)\s*\*\s*(\w+)", decl).groups()
            members.append((name, ctype))
    assert [m[0] for m in members] == [f[0] for f in _lib.MMXTrajectory._fields_]
    assert len(members) == 8
    assert all(f[1] is C.c_void_p for f in _lib.MMXTrajectory._fields_)
    assert C.sizeof(_lib.MMXTrajectory) == 8 * C.sizeof(C.c_void_p)
    # the binding's widths and dtypes name the same arrays, with the header's element types
    assert list(_lib.TRAJ_FIELDS) == [m[0] for m in members]
    for name, ctype in members:
        assert _lib.TRAJ_FIELDS[name][1] == {"float": "float32", "int32_t": "int32"}[ctype]
    widths = {n: int(w) for n, w in re.findall(r"(\w+);\s*/\* \[T\]\[N\]\[(\d+)\]", _header())}
    widths["reward"] = 1
    assert {n: w for n, (w, _) in _lib.TRAJ_FIELDS.items()} == widths


def test_null_sim_is_refused():
    from mujoco_manip_amd import _lib

    L = _lib.load()
    rec = _lib.MMXTrajectory()
    buf = (C.c_float * 4)()
    assert L.mmx_rollout_actions(None, C.cast(buf, C.c_void_p), 4, 1, C.byref(rec)) == -1
    assert L.mmx_rollout_actions(None, C.cast(buf, C.c_void_p), 4, 1, None) == -1
    assert L.mmx_rollout_expert_record(None, 1, C.byref(rec)) == -1
    assert L.mmx_rollout_expert_record(None, 1, None) == -1
