"""Snapshot / restore at the C-ABI boundary, without a GPU: the three entry points are declared in the
reference-boundary header, exported and bound; a NULL sim is refused; and the record layout the header
documents is the binding's SNAPSHOT_FIELDS table, built from the same constants tests/test_abi.py checks."""
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmx_snapshot_bytes", "mmx_snapshot", "mmx_restore")
DTYPES = {"fp32": "float32", "int32": "int32", "uint32": "uint32", "uint64": "uint64"}


def header(name):
    return open(os.path.join(REPO, "include", name)).read()


def declared(src):
    return set(re.findall(r"^\s*(?:int|int64_t|void|const char\*|uint32_t)\s+(mmx_\w+)\s*\(", src, re.M))


def test_symbols_declared_exported_and_bound():
    from mujoco_manip_amd import _lib

    api, tuning = declared(header("mmx_api.h")), declared(header("mmx_tuning.h"))
    L = _lib.load()
    for n in NAMES:
        assert n in api and n not in tuning, n
        assert hasattr(L, n), f"libmmx.so does not export {n}"
        assert n in _lib.EXPORTED
    # no reference counterpart, and the header says so
    assert re.search(r"Snapshot and restore[^/]*no reference counterpart", header("mmx_api.h"))


def test_null_sim_is_refused():
    from mujoco_manip_amd import _lib

    L = _lib.load()
    assert L.mmx_snapshot_bytes(None) == -1
    buf = np.zeros(4096, np.uint8)  # never touched: the calls return before any launch
    assert L.mmx_snapshot(None, buf.ctypes.data, 1248) == -1
    assert L.mmx_restore(None, buf.ctypes.data, 1248, 1, None) == -1
    assert not buf.any()


def test_snapshot_fields_are_the_headers_record():
    from mujoco_manip_amd import _lib

    hdr = header("mmx_api.h")
    rows = re.findall(r"^ \*     (\w+)\s+\[(\d+)\] (\w+)", hdr, re.M)
    assert [r[0] for r in rows] == [f[0] for f in _lib.SNAPSHOT_FIELDS], "names, in the header's order"
    assert [(int(w), DTYPES[t]) for _, w, t in rows] == [(w, t) for _, w, t in _lib.SNAPSHOT_FIELDS]
    # the widths are the binding's constants, not literals that could drift from them
    want = {"rng": 4, "rng32": 1, "qpos": _lib.NQ, "qvel": _lib.NV, "ctrl": _lib.NU, "qacc_warmstart": _lib.NV,
            "kin": _lib.KIN_N, "target": 4, "episode_i": _lib.EPI_N, "episode_f": _lib.EPF_N, "obs": _lib.NOBS,
            "reward": 1, "reward_components": 6, "done": 3, "rpose": _lib.RPOSE_N}
    assert {n: w for n, w, _ in _lib.SNAPSHOT_FIELDS} == want
    assert _lib.SNAPSHOT_FIELDS[-1][0] == "rpose"  # the optional field is the last
    # every field the trajectory record and the buffer struct share has the same width and dtype there
    for n, w, t in _lib.SNAPSHOT_FIELDS:
        if n in _lib.TRAJ_FIELDS:
            assert _lib.TRAJ_FIELDS[n] == (w, t), n

    def total(fields):
        return -(-sum(w * np.dtype(t).itemsize for _, w, t in fields) // 16) * 16

    plain, cams = total(_lib.SNAPSHOT_FIELDS[:-1]), total(_lib.SNAPSHOT_FIELDS)
    assert f"#define MMX_SNAPSHOT_BYTES {plain}\n" in hdr and f"#define MMX_SNAPSHOT_BYTES_CAMERAS {cams}\n" in hdr
    assert (_lib.snapshot_record_bytes(False), _lib.snapshot_record_bytes(True)) == (plain, cams)
    assert plain % 16 == 0 and cams % 16 == 0 and cams > plain
    # offsets: packed, rng first (64-bit words), rpose at the padded end of the rest (16-byte words)
    off = _lib.snapshot_field_offsets(True)
    assert off["rng"][0] == 0 and off["rpose"][0] == plain and off["rpose"][0] + 4 * _lib.RPOSE_N == cams
    assert "rpose" not in _lib.snapshot_field_offsets(False)
    end = 0
    for n, _, _ in _lib.SNAPSHOT_FIELDS[:-1]:
        o, w, t = off[n]
        assert o == end and o % np.dtype(t).itemsize == 0, n
        end = o + w * np.dtype(t).itemsize
    # the kernel source asserts the same two sizes at compile time
    src = open(os.path.join(REPO, "mujoco_manip_amd", "csrc", "mmx_snapshot.hip")).read()
    assert f"kFixedBytes == {plain} && kCameraBytes == {cams}" in src
