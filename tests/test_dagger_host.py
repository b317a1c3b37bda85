"""The DAgger gate's closed forms (csrc/mmx_dagger.h: the code mmx_env_dagger_kernel runs) on the host, under
AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU; the Python layer's validation; the C-ABI boundary.

tests/host/mmx_dagger_selftest.cpp is built here with g++ and the sanitizers and run as a child process; nothing is
loaded into python under a sanitizer.  Checked: the gate's uniform on a grid of (seed, call, t, i) against the
Philox restatement (tests/dagger_ref.py on tests/mppi_ref.py), bit for bit, in [0, 1), and different from both
uniforms of every noise component's block of the same (t, i); beta 0 and 1 never and always fire; the takeover
predicate on hand cases either side of the threshold; the gate word and the executed action."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dagger_ref
import mppi_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "mmx_dagger_selftest.cpp")
_EXE = {}


def run(tmp_path_factory, *args):
    if "exe" not in _EXE:
        assert shutil.which("g++"), "this test needs g++ (the sanitizer build of the host program)"
        exe = str(tmp_path_factory.mktemp("dagger_host") / "mmx_dagger_selftest")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], check=True, capture_output=True, timeout=300)
        _EXE["exe"] = exe
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([_EXE["exe"]] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return [json.loads(x) for x in r.stdout.splitlines()]


def f32(words):
    return np.array(words, np.uint32).view(np.float32)


GRID = [(seed, call, t, i) for seed in (0, 77, 2**64 - 1, 0x123456789ABCDEF0) for call in (0, 1, 2**32, 2**64 - 1)
        for t in (0, 1, 63, 10**6) for i in (0, 1, 9, 4095, 2**31 + 5)]


# ------------------------------------------------------------------ the draw
def test_gate_uniform_is_the_philox_word(tmp_path_factory):
    lines = run(tmp_path_factory, "draw", *[v for g in GRID for v in g])
    assert len(lines) == len(GRID)
    got = f32([x["u"] for x in lines])
    want = np.array([dagger_ref.gate_uniform(*g) for g in GRID])
    assert (got.astype(np.float64) == want).all()  # 24 bits times 2^-24: exact in fp32
    assert (got >= 0).all() and (got < 1).all() and len(set(got.tolist())) > 0.99 * len(GRID)
    assert (got * 2.0 ** 24 == np.round(got * 2.0 ** 24)).all()
    # the block is the step's fourth counter word, which no noise component (a < 10: words 4 t .. 4 t + 2) uses:
    # the restatement of the noise draw gives the program's noise uniforms, and u is none of them
    for g, x in zip(GRID[::7], lines[::7]):
        noise = f32(x["noise"]).reshape(10, 2)
        for a in range(10):
            u1, u2, _ = mppi_ref.draw(*g, a)
            assert noise[a, 0] == u1 and noise[a, 1] == u2, (g, a)
    for x, u in zip(lines, got):
        assert u not in f32(x["noise"]), x
    # (seed, call, t, i) each matter
    base = dagger_ref.gate_uniform(77, 0, 3, 5)
    assert len({base, dagger_ref.gate_uniform(78, 0, 3, 5), dagger_ref.gate_uniform(77, 1, 3, 5), dagger_ref.gate_uniform(77, 0, 4, 5),
                dagger_ref.gate_uniform(77, 0, 3, 6)}) == 5


def gate_lines(tmp_path_factory, cases):
    """cases: (seed, call, t, i, beta, tau, policy [4], expert [4])."""
    args = []
    for seed, call, t, i, beta, tau, p, e in cases:
        args += [seed, call, t, i, repr(float(beta)), repr(float(tau))] + [repr(float(v)) for v in list(p) + list(e)]
    return run(tmp_path_factory, "gate", *args)


def test_beta_zero_never_fires_and_one_always(tmp_path_factory):
    p, e = (0.1, 0.4, 0.5, 1.0), (-0.1, 0.3, 0.4, 0.0)
    keys = GRID[::3]
    for beta, bit in ((0.0, 0), (1.0, 1)):
        lines = gate_lines(tmp_path_factory, [(*g, beta, 0.0, p, e) for g in keys])
        assert [x["bern"] for x in lines] == [bit] * len(keys) and [x["gate"] for x in lines] == [bit] * len(keys)
        want = e if bit else p
        for x in lines:
            assert (f32(x["action"]) == np.array(want, np.float32)).all()
    # in between: the bit is u < beta on the program's own u, and both outcomes occur
    lines = gate_lines(tmp_path_factory, [(*g, 0.5, 0.0, p, e) for g in GRID])
    u = f32([x["u"] for x in lines])
    bern = np.array([x["bern"] for x in lines])
    assert (bern == (u < 0.5)).all() and 0.3 < bern.mean() < 0.7
    # the smallest and the largest u there is: 0 fires for any beta > 0, 1 - 2^-24 only for beta = 1
    assert dagger_ref.gate_uniform(0, 0, 0, 0) < 1.0


def test_takeover_either_side_of_the_threshold(tmp_path_factory):
    e = (0.0, 0.4, 0.5, 1.0)
    key = (77, 0, 2, 3)
    tau = 0.05
    cases = [
        ((0.0, 0.4, 0.5, 0.0), tau, 0),            # the same xyz; the gripper component never counts
        ((0.049, 0.4, 0.5, 1.0), tau, 0),          # inside, along x
        ((0.051, 0.4, 0.5, 1.0), tau, 1),          # outside, along x
        ((0.0, 0.4 - 0.051, 0.5, 1.0), tau, 1),    # along y, the other sign
        ((0.0, 0.4, 0.5 + 0.049, 1.0), tau, 0),    # along z
        ((0.03, 0.43, 0.53, 1.0), tau, 1),         # 0.03 sqrt 3 = 0.052
        ((0.028, 0.428, 0.528, 1.0), tau, 0),      # 0.028 sqrt 3 = 0.0485
        ((0.05, 0.4, 0.5, 1.0), tau, 0),           # on the threshold: fl(0.05)^2 against fl(0.05)^2, "greater" is strict
        ((5.0, 5.0, 5.0, 0.0), 0.0, 0),            # takeover_dist = 0 switches it off, however far
        ((5.0, 5.0, 5.0, 0.0), 1e-30, 1),          # a tiny threshold is on
    ]
    lines = gate_lines(tmp_path_factory, [(*key, 0.0, t, p, e) for p, t, _ in cases])
    for (p, t, want), x in zip(cases, lines):
        assert x["take"] == want and x["gate"] == want << 1 and x["bern"] == 0, (p, t, x)
        assert f32([x["d2"]])[0] == dagger_ref.dist2_f32(p, e), (p, x)
        assert (f32(x["action"]) == np.array(e if want else p, np.float32)).all()
    # both bits at once
    (x,) = gate_lines(tmp_path_factory, [(*key, 1.0, tau, (0.3, 0.4, 0.5, 0.0), e)])
    assert x["gate"] == 3 and (f32(x["action"]) == np.array(e, np.float32)).all()


# ------------------------------------------------------------------ the Python layer, without a GPU
def test_rollout_dagger_argument_validation():
    import mujoco_manip_amd
    from mujoco_manip_amd import _lib, dagger

    assert mujoco_manip_amd.DaggerBuffer is dagger.DaggerBuffer and "DaggerBuffer" in mujoco_manip_amd.__all__
    assert dagger.check_args(5, 0.5, 0.0, ("obs_in", "gate", "obs")) == (5, 0.5, 0.0, ("obs_in", "gate", "obs"))
    assert dagger.check_args(0, 1, 0.25, "gate") == (0, 1.0, 0.25, ("gate",))
    assert dagger.check_args(np.int64(3), 0, 0, None) == (3, 0.0, 0.0, ())
    assert set(dagger.DEFAULT_RECORD) <= set(_lib.TRAJ_FIELDS) | set(_lib.DAGGER_FIELDS)
    for beta in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beta"):
            dagger.check_args(5, beta, 0.0, ())
    for tau in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="takeover_dist"):
            dagger.check_args(5, 0.5, tau, ())
    for n in (-1, None, 2.5):
        with pytest.raises(ValueError, match="n_steps"):
            dagger.check_args(n, 0.5, 0.0, ())
    with pytest.raises(ValueError, match="record entries"):
        dagger.check_args(5, 0.5, 0.0, ("obs", "images"))


def test_dagger_buffer_on_the_host():
    torch = pytest.importorskip("torch")
    from mujoco_manip_amd.dagger import DaggerBuffer

    def rec(T, N, base):
        obs = torch.arange(T * N * 85, dtype=torch.float32).reshape(T, N, 85) + base
        return {"obs_in": obs, "expert_action": obs[:, :, :4] * 2, "gate": torch.zeros(T, N, dtype=torch.int32)}

    a, b = rec(3, 2, 0.0), rec(2, 2, 1e6)
    buf = DaggerBuffer()
    assert len(buf) == 0 and buf.tensors() == (None, None)
    assert buf.add(a) == 6 and buf.add(b) == 10
    obs, lab = buf.tensors()
    assert torch.equal(obs, torch.cat([a["obs_in"].reshape(-1, 85), b["obs_in"].reshape(-1, 85)]))  # (t, i) order
    assert torch.equal(obs[1], a["obs_in"][0, 1]) and torch.equal(obs[2], a["obs_in"][1, 0])
    assert torch.equal(lab, obs[:, :4] * 2) and buf.dropped == 0
    small = DaggerBuffer(capacity=7)
    small.add(a)
    small.add(b)
    so, sl = small.tensors()
    assert len(small) == 7 and small.dropped == 3 and torch.equal(so, obs[3:]) and torch.equal(sl, lab[3:])
    small.add(rec(4, 2, 2e6))  # one add larger than the capacity: its newest pairs
    assert len(small) == 7 and torch.equal(small.tensors()[0], rec(4, 2, 2e6)["obs_in"].reshape(-1, 85)[1:])
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="capacity"):
            DaggerBuffer(capacity=bad)
    with pytest.raises(ValueError, match="obs_in"):
        buf.add({"obs": a["obs_in"]})
    with pytest.raises(ValueError, match="must be"):
        buf.add({"obs_in": a["obs_in"], "expert_action": b["expert_action"]})


# ------------------------------------------------------------------ the C-ABI boundary
def test_abi_declared_exported_bound_and_laid_out(tmp_path):
    from mujoco_manip_amd import _lib
    import test_abi

    api = open(os.path.join(REPO, "include", "mmx_api.h")).read()
    assert re.search(r"^int\s+mmx_rollout_dagger\s*\(", api, re.M)
    assert "mmx_rollout_dagger" in test_abi.declared_functions(("mmx_api.h",)) and "mmx_rollout_dagger" in _lib.EXPORTED
    L = _lib.load()
    assert hasattr(L, "mmx_rollout_dagger")
    test_abi.test_library_exports_every_declared_symbol()
    test_abi.test_reference_boundary_header_has_no_tuning_entry_points()
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "this test needs a C compiler"
    config, record = ("beta", "takeover_dist"), ("actions", "expert_action", "policy_action", "mean", "noise", "gate", "obs_in")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "mmx_api.h"', "int main(void) {",
             '  printf("{\\"config\\": %zu, \\"record\\": %zu", sizeof(mmx_dagger_config), sizeof(mmx_dagger_record));']
    for struct, names in (("mmx_dagger_config", config), ("mmx_dagger_record", record)):
        for n in names:
            lines.append(f'  printf(", \\"{struct}.{n}\\": %zu", offsetof({struct}, {n}));')
    lines += ['  printf("}\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, timeout=120)
    got = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout)
    assert [f[0] for f in _lib.MMXDaggerConfig._fields_] == list(config)
    assert [f[0] for f in _lib.MMXDaggerRecord._fields_] == list(record) == list(_lib.DAGGER_FIELDS)
    assert C.sizeof(_lib.MMXDaggerConfig) == got["config"] and C.sizeof(_lib.MMXDaggerRecord) == got["record"]
    for n in config:
        assert getattr(_lib.MMXDaggerConfig, n).offset == got[f"mmx_dagger_config.{n}"], n
    for n in record:
        assert getattr(_lib.MMXDaggerRecord, n).offset == got[f"mmx_dagger_record.{n}"], n
    # NULL arguments are refused before anything is touched
    buf = (C.c_float * 64)()
    drec = _lib.MMXDaggerRecord(actions=C.cast(buf, C.c_void_p).value)
    cfg = _lib.MMXDaggerConfig(beta=0.5, takeover_dist=0.0)
    assert L.mmx_rollout_dagger(None, None, 3, 0, C.byref(cfg), C.byref(drec), None) == -1
    assert L.mmx_rollout_dagger(None, None, 0, 0, None, None, None) == -1
    assert not any(buf)
