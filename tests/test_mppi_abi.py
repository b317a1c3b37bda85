"""The MPPI planner's C-ABI boundary, without a GPU: the five entry points are declared in include/mmx_api.h,
exported and bound; the binding's two ctypes structures have the sizes and member offsets of the header's
structs (read from a tiny C program compiled against the header); the two constants agree; NULL arguments are
refused; and mujoco_manip_amd.planner imports without a GPU."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mmx_mppi_create", "mmx_mppi_destroy", "mmx_mppi_reset", "mmx_mppi_plan", "mmx_mppi_get_buffers",
           "mmx_mppi_reweight")
CONFIG = ("horizon", "samples", "temperature", "discount", "noise_beta", "sigma", "low", "high", "seed")
BUFFERS = ("nominal", "noise", "actions", "reward", "done", "returns", "weights", "best")


def _header():
    return open(os.path.join(REPO, "include", "mmx_api.h")).read()


def test_symbols_declared_exported_and_bound():
    from mujoco_manip_amd import _lib

    api = _header()
    L = _lib.load()
    for sym in SYMBOLS:
        assert re.search(rf"^(?:int|void)\s+{sym}\s*\(", api, re.M), f"{sym} not declared in mmx_api.h"
        assert hasattr(L, sym), f"libmmx.so does not export {sym}"
        assert sym in _lib.EXPORTED
    assert re.search(r"MPPI planning on the device[^/]*no reference counterpart", api)


def test_structs_and_constants_match_the_header(tmp_path):
    from mujoco_manip_amd import _lib

    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "this test needs a C compiler"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "mmx_api.h"', "int main(void) {",
             '  printf("{\\"config\\": %zu, \\"buffers\\": %zu, \\"horizon_max\\": %d, \\"adim_max\\": %d",',
             "         sizeof(mmx_mppi_config), sizeof(mmx_mppi_buffers), MMX_MPPI_MAX_HORIZON, MMX_MPPI_MAX_ADIM);"]
    for struct, names in (("mmx_mppi_config", CONFIG), ("mmx_mppi_buffers", BUFFERS)):
        for n in names:
            lines.append(f'  printf(", \\"{struct}.{n}\\": %zu", offsetof({struct}, {n}));')
    lines += ['  printf("}\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, timeout=120)
    got = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout)
    assert [f[0] for f in _lib.MMXMppiConfig._fields_] == list(CONFIG)
    assert [f[0] for f in _lib.MMXMppiBuffers._fields_] == list(BUFFERS)
    assert C.sizeof(_lib.MMXMppiConfig) == got["config"] and C.sizeof(_lib.MMXMppiBuffers) == got["buffers"]
    for n in CONFIG:
        assert getattr(_lib.MMXMppiConfig, n).offset == got[f"mmx_mppi_config.{n}"], n
    for n in BUFFERS:
        assert getattr(_lib.MMXMppiBuffers, n).offset == got[f"mmx_mppi_buffers.{n}"], n
    assert (_lib.MPPI_MAX_HORIZON, _lib.MPPI_MAX_ADIM) == (got["horizon_max"], got["adim_max"]) == (64, 10)
    assert max(_lib.ACTION_DIMS) <= _lib.MPPI_MAX_ADIM
    # the kernels' header carries the same two limits
    src = open(os.path.join(REPO, "mujoco_manip_amd", "csrc", "mmx_mppi.h")).read()
    assert "#define MPPI_MAX_HORIZON 64 " in src and "#define MPPI_MAX_ADIM 10 " in src


def test_null_arguments_are_refused():
    from mujoco_manip_amd import _lib

    L = _lib.load()
    cfg, ptr, bufs = _lib.MMXMppiConfig(horizon=3, samples=8, temperature=1.0, discount=1.0), C.c_void_p(), _lib.MMXMppiBuffers()
    buf = (C.c_float * 64)()
    assert L.mmx_mppi_create(None, C.byref(cfg), C.byref(ptr)) == -1 and not ptr.value
    assert L.mmx_mppi_reset(None, C.cast(buf, C.c_void_p)) == -1
    assert L.mmx_mppi_plan(None, C.cast(buf, C.c_void_p), 1248, 1, None, C.cast(buf, C.c_void_p)) == -1
    assert L.mmx_mppi_get_buffers(None, C.byref(bufs)) == -1
    assert L.mmx_mppi_reweight(None, C.cast(buf, C.c_void_p)) == -1
    L.mmx_mppi_destroy(None)  # a no-op
    assert not any(buf)


def test_planner_imports_without_a_gpu():
    import mujoco_manip_amd
    from mujoco_manip_amd import planner

    assert mujoco_manip_amd.MppiPlanner is planner.MppiPlanner
    assert "MppiPlanner" in mujoco_manip_amd.__all__
    low, high = planner.action_box("abs_pos")
    assert low == [-0.5, 0.0, float(np.float32(0.24)), 0.0] and high == [0.5, float(np.float32(0.8)), float(np.float32(0.6)), 1.0]
    low, high = planner.action_box("ee_pos_rot6d_g")
    assert len(low) == 10 and all(abs(v) < float("inf") for v in low + high) and (low[9], high[9]) == (0.0, 1.0)
