"""The MLP policy's C-ABI boundary, without a GPU: the four entry points are declared in include/mmx_api.h,
exported and bound; the binding's two ctypes structures have the sizes and member offsets of the header's structs
(read from a tiny C program compiled against the header); the constants agree with the binding and with the
kernels' header; NULL arguments are refused."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mmx_policy_create", "mmx_policy_destroy", "mmx_policy_eval", "mmx_rollout_policy")
CONFIG = ("n_layers", "width", "activation", "weight", "bias", "obs_shift", "obs_scale", "log_std", "low", "high", "seed")
RECORD = ("actions", "mean", "noise")


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
    assert re.search(r"Closed-loop MLP policies[^/]*no reference counterpart", api)


def test_structs_and_constants_match_the_header(tmp_path):
    from mujoco_manip_amd import _lib

    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "this test needs a C compiler"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "mmx_api.h"', "int main(void) {",
             '  printf("{\\"config\\": %zu, \\"record\\": %zu, \\"layers\\": %d, \\"width\\": %d, \\"tanh\\": %d, \\"relu\\": %d",',
             "         sizeof(mmx_policy_config), sizeof(mmx_policy_record), MMX_POLICY_MAX_LAYERS, MMX_POLICY_MAX_WIDTH,",
             "         MMX_POLICY_TANH, MMX_POLICY_RELU);"]
    for struct, names in (("mmx_policy_config", CONFIG), ("mmx_policy_record", RECORD)):
        for n in names:
            lines.append(f'  printf(", \\"{struct}.{n}\\": %zu", offsetof({struct}, {n}));')
    lines += ['  printf("}\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, timeout=120)
    got = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout)
    assert [f[0] for f in _lib.MMXPolicyConfig._fields_] == list(CONFIG)
    assert [f[0] for f in _lib.MMXPolicyRecord._fields_] == list(RECORD)
    assert C.sizeof(_lib.MMXPolicyConfig) == got["config"] and C.sizeof(_lib.MMXPolicyRecord) == got["record"]
    for n in CONFIG:
        assert getattr(_lib.MMXPolicyConfig, n).offset == got[f"mmx_policy_config.{n}"], n
    for n in RECORD:
        assert getattr(_lib.MMXPolicyRecord, n).offset == got[f"mmx_policy_record.{n}"], n
    assert (_lib.POLICY_MAX_LAYERS, _lib.POLICY_MAX_WIDTH) == (got["layers"], got["width"]) == (4, 256)
    assert _lib.POLICY_ACTIVATIONS.index("tanh") == got["tanh"] == 0 and _lib.POLICY_ACTIVATIONS.index("relu") == got["relu"] == 1
    # the kernels' header carries the same limits, and the observation's width
    src = open(os.path.join(REPO, "mujoco_manip_amd", "csrc", "mmx_policy.h")).read()
    for text in ("#define POLICY_MAX_LAYERS 4 ", "#define POLICY_MAX_WIDTH 256 ", f"#define POLICY_NOBS {_lib.NOBS} ",
                 "#define POLICY_TANH 0 ", "#define POLICY_RELU 1 ", "#define POLICY_MAX_ADIM MPPI_MAX_ADIM"):
        assert text in src, text


def test_null_arguments_are_refused():
    from mujoco_manip_amd import _lib

    L = _lib.load()
    cfg, ptr = _lib.MMXPolicyConfig(n_layers=1), C.c_void_p()
    cfg.width[0] = 4
    buf = (C.c_float * 512)()
    cfg.weight[0] = C.cast(buf, C.c_void_p).value
    prec = _lib.MMXPolicyRecord(actions=C.cast(buf, C.c_void_p).value)
    assert L.mmx_policy_create(None, C.byref(cfg), C.byref(ptr)) == -1 and not ptr.value
    assert L.mmx_policy_create(None, None, None) == -1
    assert L.mmx_policy_eval(None, C.cast(buf, C.c_void_p), 1, C.cast(buf, C.c_void_p)) == -1
    assert L.mmx_rollout_policy(None, None, 3, 0, C.byref(prec), None) == -1
    L.mmx_policy_destroy(None)  # a no-op
    assert not any(buf)
