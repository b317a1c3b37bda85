"""The MLP policy's closed forms (csrc/mmx_policy.h: the code the kernels run) on the host, under
AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU, and the Python layer's validation.

tests/host/mmx_policy_selftest.cpp is built here with g++ and the sanitizers and run as a child process; nothing is
loaded into python under a sanitizer.  Checked: the packed layout at widths 1, 63, 64, 65 and 256 in a blob of
exactly the computed size; the scalar forward pass against the fp64 restatement of tests/policy_ref.py within its
forward-error bound (the host's exp2f and division are at least as accurate as the hardware forms the bound is
made for); tanh's saturation and its value at 0; the action formula and its clamp."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from policy_ref import ACT_EPS, U, forward64, make_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "mmx_policy_selftest.cpp")
_EXE = {}


def run(tmp_path_factory, *args):
    if "exe" not in _EXE:
        assert shutil.which("g++"), "this test needs g++ (the sanitizer build of the host program)"
        exe = str(tmp_path_factory.mktemp("policy_host") / "mmx_policy_selftest")
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


def test_packed_layout(tmp_path_factory):
    lines = run(tmp_path_factory, "pack")
    assert {(x["in"], x["out"]) for x in lines} == {(i, o) for i in (1, 85, 256) for o in (1, 63, 64, 65, 256)}
    for x in lines:
        padded = -(-x["out"] // 64) * 64
        assert x["wrong"] == 0 and x["padded"] == padded
        assert x["layer_floats"] == (x["in"] + 1) * padded and x["floats"] == x["layer_floats"] + 2 * 85 + 3 * 10


def write_case(path, spec, obs):
    with open(path, "w") as f:
        f.write(f"{len(spec['layers'])} {('tanh', 'relu').index(spec['activation'])} {len(obs)}\n")
        f.write(" ".join(str(W.shape[0]) for W, _ in spec["layers"]) + "\n")
        for W, b in spec["layers"]:
            f.write(f"{int(b is not None)}\n" + " ".join(repr(float(v)) for v in W.ravel()) + "\n")
            if b is not None:
                f.write(" ".join(repr(float(v)) for v in b) + "\n")
        for arr in (spec["obs_shift"], spec["obs_scale"], obs):
            f.write(" ".join(repr(float(v)) for v in arr.ravel()) + "\n")


@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("hidden,A,bias", [((), 4, True), ((63,), 10, False), ((65, 64), 4, True), ((256, 1, 255), 10, True)])
def test_scalar_forward_against_fp64(tmp_path_factory, hidden, A, bias, activation):
    spec = make_spec(A, hidden=hidden, activation=activation, bias=bias, seed=len(hidden) + A)
    spec["obs_scale"][17] = 0.0
    obs = np.random.default_rng(3).uniform(-2.0, 2.0, (5, 85)).astype(np.float32)
    obs[:, 17] = np.float32(3e30)  # dropped by the zero scale
    path = str(tmp_path_factory.mktemp("policy_case") / "case.txt")
    write_case(path, spec, obs)
    (x,) = run(tmp_path_factory, "forward", path)
    got = f32(x["mean"]).reshape(5, A)
    want, bound = forward64(spec, obs)
    frac = (np.abs(got.astype(np.float64) - want) / np.maximum(bound, 1e-300)).max()
    print("worst fraction of the forward-error bound:", frac)
    assert np.isfinite(got).all() and frac <= 1.0 and np.abs(want).max() < 1e3


def test_tanh_saturates(tmp_path_factory):
    grid = [0.0] + [s * 2.0 ** e for e in range(-20, 5) for s in (1, -1)] + [s * v for v in (20.0, 88.0, 100.0, 1e30) for s in (1, -1)]
    lines = run(tmp_path_factory, "tanh", *[repr(v) for v in grid])
    got = f32([x["y"] for x in lines])
    assert len(got) == len(grid) and ((got.view(np.uint32) & 0x7F800000) != 0x7F800000).all()
    err = np.abs(got.astype(np.float64) - np.tanh(np.array(grid))).max()
    print("host tanh: max error / ACT_EPS =", err / ACT_EPS)
    assert err <= ACT_EPS
    for v, y in zip(grid, got):
        if abs(v) >= 20.0:
            assert y == np.sign(v), (v, y)
    assert got[0] == 0.0


def test_action_formula_and_clamp(tmp_path_factory):
    cases = [(0.3, 0.05, 1.5, -0.5, 0.5), (0.49, 0.05, 1.5, -0.5, 0.5), (-0.49, 0.1, -2.0, -0.5, 0.5), (0.2, 0.0, 9.0, 0.0, 1.0),
             (7.0, 1.0, 0.0, -3.4028234663852886e38, 3.4028234663852886e38), (0.0, 0.5, -4.0, 0.0, 1.0)]
    lines = run(tmp_path_factory, "action", *[repr(v) for c in cases for v in c])
    got = f32([x["y"] for x in lines])
    for (m, s, z, lo, hi), y in zip(cases, got):
        m, s, z = (np.float64(np.float32(v)) for v in (m, s, z))
        want = np.clip(np.float32(s * z + m), np.float32(lo), np.float32(hi))  # one rounding: the fused form
        assert y == want, (m, s, z, lo, hi, y, want)
    assert got[1] == np.float32(0.5) and got[2] == np.float32(-0.5) and got[4] == 7.0 and got[5] == 0.0
    assert abs(float(got[0]) - 0.375) <= 2 * U


# ------------------------------------------------------------------ the Python layer, without a GPU
def test_policy_module_imports_without_a_gpu():
    import mujoco_manip_amd
    from mujoco_manip_amd import policy

    assert mujoco_manip_amd.MlpPolicy is policy.MlpPolicy and "MlpPolicy" in mujoco_manip_amd.__all__


def test_mlp_policy_validation():
    from mujoco_manip_amd.policy import MlpPolicy

    W1, W2 = np.zeros((16, 85), np.float32), np.zeros((4, 16), np.float32)
    p = MlpPolicy([(W1, np.zeros(16)), (W2, None)], log_std=np.zeros(4), low=[0] * 4, high=[1] * 4)
    assert p.action_dim == 4 and p.layers[0][1].dtype == np.float32 and p.layers[1][1] is None
    for bad in ([(np.zeros((16, 84), np.float32), None), (W2, None)],        # not 85 inputs
                [(W1, None), (np.zeros((4, 15), np.float32), None)],         # does not chain
                [(W1, np.zeros(15)), (W2, None)],                            # bias of the wrong length
                [(np.zeros((257, 85), np.float32), None), (np.zeros((4, 257), np.float32), None)],  # too wide
                [(W1, None)] + [(np.zeros((16, 16), np.float32), None)] * 3 + [(W2, None)],          # five layers
                [(W1, None), (np.zeros((11, 16), np.float32), None)],        # more outputs than an action has
                [], [(np.zeros(85, np.float32), None)]):
        with pytest.raises(ValueError):
            MlpPolicy(bad)
    with pytest.raises(ValueError, match="activation"):
        MlpPolicy([(W1, None), (W2, None)], activation="gelu")
    for kw in ({"obs_shift": np.zeros(84)}, {"obs_scale": np.zeros((85, 1))}, {"log_std": np.zeros(5)}, {"low": np.zeros(3)},
               {"high": np.zeros(10)}):
        with pytest.raises(ValueError, match="must have shape"):
            MlpPolicy([(W1, None), (W2, None)], **kw)
    with pytest.raises(RuntimeError, match="not bound"):
        p.eval(np.zeros((2, 85), np.float32))
    p.close()  # a no-op on an unbound policy


def test_from_torch():
    torch = pytest.importorskip("torch")
    from mujoco_manip_amd.policy import MlpPolicy

    nn = torch.nn
    net = nn.Sequential(nn.Linear(85, 32), nn.ReLU(), nn.Linear(32, 8, bias=False), nn.ReLU(), nn.Linear(8, 4))
    p = MlpPolicy.from_torch(net, obs_shift=torch.zeros(85), seed=3)
    assert p.activation == "relu" and [W.shape for W, _ in p.layers] == [(32, 85), (8, 32), (4, 8)]
    assert p.layers[1][1] is None and (p.layers[0][0] == net[0].weight.detach().numpy()).all()
    assert (p.layers[2][1] == net[4].bias.detach().numpy()).all() and p.seed == 3
    assert MlpPolicy.from_torch(nn.Sequential(nn.Linear(85, 4))).activation == "tanh"
    assert MlpPolicy.from_torch(nn.Sequential(nn.Linear(85, 9), nn.Tanh(), nn.Linear(9, 4))).activation == "tanh"
    for bad in (nn.Sequential(nn.Linear(85, 9), nn.Tanh()), nn.Sequential(nn.Linear(85, 9), nn.Sigmoid(), nn.Linear(9, 4)),
                nn.Sequential(nn.Linear(85, 9), nn.Linear(9, 4), nn.Linear(4, 4)),
                nn.Sequential(nn.Linear(85, 9), nn.Tanh(), nn.Linear(9, 9), nn.ReLU(), nn.Linear(9, 4))):
        with pytest.raises(ValueError, match="from_torch"):
            MlpPolicy.from_torch(bad)
    # the fp64 restatement agrees with torch's own forward pass on the converted weights
    x = torch.randn(6, 85)
    spec = dict(layers=p.layers, activation=p.activation, obs_shift=np.zeros(85, np.float32), obs_scale=np.ones(85, np.float32))
    want, bound = forward64(spec, x.numpy())
    assert np.abs(net(x).detach().numpy() - want).max() <= 4 * bound.max()
