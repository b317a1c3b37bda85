"""The closed forms of the policy-gradient fit (csrc/mmx_pg.h: the code the kernels run) on the host, under
AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU, and the Python layer's validation.

tests/host/mmx_pg_selftest.cpp is built here with g++ and the sanitizers and run as a child process, as
tests/test_policy_fit_host.py does with its program; nothing is loaded into python under a sanitizer.  Checked: the
fp64 restatement of tests/pg_ref.py against torch.autograd in float64 (the clipped surrogate with
torch.distributions.Normal log-probabilities); the scalar reference step against that restatement (one SGD step at
lr = 1, so the weight change is the gradient) within the gate the GPU test uses; GAE and the normalisation against the
fp64 recursion; the two new structs' layout; refusals without a device; fit_pg's, gae's and MlpCritic's validation."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import pg_ref as R
from policy_ref import make_spec
from test_policy_fit_host import _Untouched, f32, words, write_case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "mmx_pg_selftest.cpp")
_EXE = {}
F32 = np.float32
CLIP = 0.2


def run(tmp_path_factory, *args):
    if "exe" not in _EXE:
        assert shutil.which("g++"), "this test needs g++ (the sanitizer build of the host program)"
        exe = str(tmp_path_factory.mktemp("pg_host") / "mmx_pg_selftest")
        # -ffp-contract=off: the operation order is stated one rounding at a time
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], check=True, capture_output=True, timeout=300)
        _EXE["exe"] = exe
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([_EXE["exe"]] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return [json.loads(x) for x in r.stdout.splitlines()]


def gate(name, got, want64, yard):
    e, y = R.err(got, want64), R.err(yard, want64)
    frac = e / (8 * max(y, R.U))
    assert frac <= 1.0, f"{name}: err {e:.3e}, yardstick {y:.3e}, {frac:.2f} of the gate"
    return frac


# ------------------------------------------------------------------ the fp64 restatement against torch
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_fp64_restatement_against_torch(activation):
    torch = pytest.importorskip("torch")
    nn = torch.nn
    spec, case = R.make_pg_case((33, 20), 4, activation, True, 50)
    obs, mean_old, noise, adv, std = case
    spec["obs_scale"][17] = 1.0  # torch has no dropped entry; keep the input finite instead
    obs[:, 17] = 0.5
    net64 = R.PgNet(spec, False)
    act = nn.Tanh if activation == "tanh" else nn.ReLU
    tnet = nn.Sequential(nn.Linear(85, 33), act(), nn.Linear(33, 20), act(), nn.Linear(20, 4)).double()
    with torch.no_grad():
        for m, (W, b) in zip(list(tnet)[0::2], net64.layers):
            m.weight.copy_(torch.from_numpy(W))
            m.bias.copy_(torch.from_numpy(b))
    x = torch.from_numpy((obs.astype(np.float64) - net64.shift) * net64.scale)
    sd = torch.from_numpy(std.astype(np.float64))
    lo, hi = float(F32(1) - F32(CLIP)), float(F32(1) + F32(CLIP))
    u = torch.from_numpy(mean_old.astype(np.float64) + std.astype(np.float64) * noise.astype(np.float64))  # the pre-clamp sample
    logp_old = torch.distributions.Normal(torch.from_numpy(mean_old.astype(np.float64)), sd).log_prob(u).sum(1)
    A = torch.from_numpy(adv.astype(np.float64))
    worst, clipped = 0.0, 0
    for step in range(5):
        idx = R.batch_indices(1, 9, step, 24, len(obs))
        R.assert_clip_condition(net64, case, idx, CLIP)
        tnet.zero_grad()
        r = torch.exp(torch.distributions.Normal(tnet(x[idx]), sd).log_prob(u[idx]).sum(1) - logp_old[idx])
        loss = -torch.minimum(r * A[idx], torch.clamp(r, lo, hi) * A[idx]).mean()
        loss.backward()
        stats, grads = net64.gradients(obs[idx], (mean_old[idx], noise[idx], adv[idx], std, CLIP))
        for m, (dW, db) in zip(list(tnet)[0::2], grads):
            worst = max(worst, R.err(dW, m.weight.grad.numpy()), R.err(db, m.bias.grad.numpy()))
        rr = r.detach().numpy()
        worst = max(worst, abs(stats[0] - loss.item()) / abs(loss.item()), abs(stats[1] - np.mean((rr - 1) - np.log(rr))) / stats[1])
        clipped += int(round(stats[2] * 24))
        net64.step(obs[idx], (mean_old[idx], noise[idx], adv[idx], std, CLIP), "sgd", lr=0.05)
        with torch.no_grad():
            for m, (W, b) in zip(list(tnet)[0::2], net64.layers):
                m.weight.copy_(torch.from_numpy(W))
                m.bias.copy_(torch.from_numpy(b))
    print("fp64 restatement against torch, worst relative difference:", worst, "clipped samples:", clipped)
    assert 0 < clipped < 5 * 24  # both branches of the clip were taken
    assert worst <= 1e-12


# ------------------------------------------------------------------ the scalar reference step
def write_pg_case(path, spec, case, B, **kw):
    obs, mean_old, noise, adv, std = case
    write_case(path, spec, obs, mean_old, B, **kw)
    with open(path, "a") as f:
        for arr in (spec["log_std"], noise, adv, [CLIP]):
            f.write(words(arr) + "\n")


@pytest.mark.parametrize("B,n", [(1, 3), (15, 20), (17, 17), (33, 12)])
@pytest.mark.parametrize("hidden,A,activation,bias", [((70, 33), 4, "tanh", True), ((70, 33), 10, "relu", False), ((), 4, "tanh", True),
                                                      ((), 10, "relu", True)])
def test_scalar_step_against_fp64(tmp_path_factory, hidden, A, activation, bias, B, n):
    spec, case = R.make_pg_case(hidden, A, activation, bias, n)
    obs, mean_old, noise, adv, std = case
    idx = R.batch_indices(0, 0, 0, B, n)
    assert (n >= B) or len(set(idx)) < B  # n < B: pairs repeat
    n64, n32 = R.PgNet(spec, False), R.PgNet(spec, True)
    R.assert_clip_condition(n64, case, idx, CLIP)
    path = str(tmp_path_factory.mktemp("pg_case") / "case.txt")
    write_pg_case(path, spec, case, B)
    (x,) = run(tmp_path_factory, "step", path)
    pack = (mean_old[idx], noise[idx], adv[idx], std, CLIP)
    s64, s32 = n64.step(obs[idx], pack, "sgd", lr=1.0), n32.step(obs[idx], pack, "sgd", lr=1.0)
    before = R.Net(spec, False).layers
    assert x["pad_nonzero"] == 0 and x["outside_changed"] == 0
    worst = 0.0
    for l, (lay, (W0, b0), (W64, b64), (W32, b32)) in enumerate(zip(x["layers"], before, n64.layers, n32.layers)):
        gotW, gotb = f32(lay["W"]).reshape(W0.shape), f32(lay["b"])
        for got, w0, w64, w32 in ((gotW, W0, W64, W32), (gotb, b0, b64, b32)):
            if not np.any(w64 - w0):  # every sample clipped (B = 1): a gradient of exactly 0
                assert (got == w0.astype(F32)).all()
                continue
            worst = max(worst, gate(f"layer {l}", got.astype(np.float64) - w0, w64 - w0, w32.astype(np.float64) - w0))
        if l == 0:  # the dropped observation entry: a gradient of exactly 0
            assert (gotW[:, 17] == W0[:, 17].astype(F32)).all()
    got = f32(x["stats"])
    for c, name in enumerate(("loss", "kl", "clipped")):
        if name == "kl" and B == 1:  # one sample's (r - 1) - log r has no conditioning to speak of: pg_ref.make_pg_case
            continue
        worst = max(worst, gate(name, got[c:c + 1], s64[c:c + 1], s32[c:c + 1]))
    print("scalar reference: worst fraction of the gate:", worst)


# ------------------------------------------------------------------ GAE
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("T,N", R.GAE_SHAPES + [(3, 1500)])
def test_gae_against_fp64(tmp_path_factory, T, N, normalize):
    reward, done, value, value_last = R.make_gae_case(T, N)
    path = str(tmp_path_factory.mktemp("gae_case") / "case.txt")
    with open(path, "w") as f:
        f.write(f"{T} {N} {normalize} {words([0.99, 0.95])}\n{words(reward)}\n" + " ".join(str(int(v)) for v in done.ravel()) + "\n")
        f.write(f"{words(value)}\n{words(value_last)}\n")
    (x,) = run(tmp_path_factory, "gae", path)
    (a64, r64), (a32, r32) = (R.gae(reward, done, value, value_last, 0.99, 0.95, f) for f in (False, True))
    if normalize:
        a64, a32 = R.normalise(a64, False), R.normalise(a32, True)
    adv, ret = f32(x["adv"]).reshape(T, N), f32(x["ret"]).reshape(T, N)
    worst = max(gate("adv", adv, a64, a32), gate("ret", ret, r64, r32))
    # an ended step's advantage is its own delta: nothing behind it enters
    end = (done[..., 0] != 0) | (done[..., 1] != 0)
    if not normalize and end.any():
        assert (adv[end] == (reward[end] - value[end])).all()
    print("gae: worst fraction of the gate:", worst)


# ------------------------------------------------------------------ the Python layer, without a GPU
def test_fit_pg_validation():
    torch = pytest.importorskip("torch")
    from mujoco_manip_amd import _lib
    from mujoco_manip_amd.policy import MlpPolicy

    spec = make_spec(4, hidden=(16,))
    p = MlpPolicy(spec["layers"], log_std=np.zeros(4, F32))
    obs, mo, z, adv = torch.zeros(8, 85), torch.zeros(8, 4), torch.zeros(8, 4), torch.ones(8)
    with pytest.raises(RuntimeError, match="not bound"):
        p.fit_pg(obs, mo, z, adv, 1)
    with pytest.raises(RuntimeError, match="not bound"):
        p.set_log_std(np.zeros(4))
    p._dev, p._env = _Untouched(), types.SimpleNamespace(device="cpu")
    bad = [dict(obs=obs.double()), dict(obs=torch.zeros(8, 84)), dict(mean_old=torch.zeros(8, 5)), dict(noise=torch.zeros(7, 4)),
           dict(adv=torch.ones(8, 1)), dict(adv=torch.ones(9)), dict(adv=np.ones(8, F32)), dict(noise=torch.zeros(4, 8).t()),
           dict(obs=torch.zeros(0, 85), mean_old=torch.zeros(0, 4), noise=torch.zeros(0, 4), adv=torch.zeros(0)),
           dict(steps=-1), dict(optimizer="lbfgs"), dict(batch=0), dict(batch=_lib.FIT_MAX_BATCH + 1), dict(lr=0.0), dict(lr=float("nan")),
           dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(clip=0.0), dict(clip=1.0), dict(clip=-0.2), dict(clip=float("nan"))]
    for kw in bad:
        args = dict(obs=obs, mean_old=mo, noise=z, adv=adv, steps=1)
        args.update(kw)
        with pytest.raises(ValueError):
            p.fit_pg(**args)
    for ls in (np.zeros(3), np.array([0, 0, np.nan, 0]), np.array([0, 0, np.inf, 0])):
        with pytest.raises(ValueError):
            p.set_log_std(ls)
    p._env = types.SimpleNamespace(device="meta")
    with pytest.raises(ValueError, match="must be on"):
        p.fit_pg(obs, mo, z, adv, 1)
    q = MlpPolicy(spec["layers"])  # deterministic: no likelihood ratio
    q._dev, q._env = _Untouched(), types.SimpleNamespace(device="cpu")
    with pytest.raises(ValueError, match="stochastic"):
        q.fit_pg(obs, mo, z, adv, 1)
    p._dev = p._env = q._dev = q._env = None


def test_critic_validation():
    torch = pytest.importorskip("torch")
    import mujoco_manip_amd
    from mujoco_manip_amd.policy import MlpCritic, MlpPolicy

    assert mujoco_manip_amd.MlpCritic is MlpCritic and "MlpCritic" in mujoco_manip_amd.__all__ and issubclass(MlpCritic, MlpPolicy)
    spec = make_spec(1, hidden=(16,))
    c = MlpCritic(spec["layers"], obs_shift=spec["obs_shift"], obs_scale=spec["obs_scale"])
    assert c.action_dim == 1 and c.log_std is None and c.low is None and c.high is None
    with pytest.raises(ValueError, match="1 output"):
        MlpCritic(make_spec(4, hidden=(16,))["layers"])
    with pytest.raises(TypeError):
        MlpCritic(spec["layers"], log_std=np.zeros(1))
    nn = torch.nn
    assert MlpCritic.from_torch(nn.Sequential(nn.Linear(85, 8), nn.ReLU(), nn.Linear(8, 1))).activation == "relu"
    with pytest.raises(RuntimeError, match="not bound"):
        c.eval(torch.zeros(2, 85))
    c._dev, c._env = _Untouched(), types.SimpleNamespace(device="cpu")
    with pytest.raises(ValueError):
        c.fit(torch.zeros(8, 85), torch.zeros(8), 1)  # targets are [n, 1]
    with pytest.raises(ValueError):
        c.eval(torch.zeros(2, 84))
    with pytest.raises(TypeError):
        c.fit_pg(None, None, None, None, 1)
    with pytest.raises(TypeError):
        c.set_log_std(np.zeros(1))
    c._dev = c._env = None


def test_gae_validation():
    torch = pytest.importorskip("torch")
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv.__new__(PickPlaceVecEnv)  # no device: every rejection comes before the library is touched
    env.sim, env.device = _Untouched(), torch.device("cpu")
    T, N = 3, 5
    good = dict(reward=torch.zeros(T, N), done=torch.zeros(T, N, 3, dtype=torch.int32), value=torch.zeros(T, N), value_last=torch.zeros(N))
    bad = [dict(reward=torch.zeros(T, N, 1)), dict(reward=torch.zeros(T, N).double()), dict(reward=np.zeros((T, N), F32)),
           dict(done=torch.zeros(T, N, 3)), dict(done=torch.zeros(T, N, 2, dtype=torch.int32)), dict(value=torch.zeros(T, N + 1)),
           dict(value_last=torch.zeros(N, 1)), dict(value=torch.zeros(N, T).t()), dict(reward=torch.zeros(T, 0)),
           dict(gamma=1.5), dict(gamma=-0.1), dict(gamma=float("nan")), dict(lam=1.01), dict(lam=float("nan"))]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            env.gae(**args)
    env.device = torch.device("meta")
    with pytest.raises(ValueError, match="must be on"):
        env.gae(**good)


# ------------------------------------------------------------------ the C-ABI boundary
def test_pg_abi_matches_the_header(tmp_path):
    """The three entry points are declared, exported and bound; the ctypes mirrors of mmx_gae_config and
    mmx_pg_config have the header's size and member offsets (read from a tiny C program)."""
    from mujoco_manip_amd import _lib

    api = open(os.path.join(REPO, "include", "mmx_api.h")).read()
    L = _lib.load()
    for sym in ("mmx_gae", "mmx_policy_fit_pg", "mmx_policy_set_log_std"):
        assert re.search(rf"^int\s+{sym}\s*\(", api, re.M) and hasattr(L, sym) and sym in _lib.EXPORTED, sym
    members = {"mmx_gae_config": (_lib.MMXGaeConfig, ["gamma", "lambda", "normalize"]), "mmx_pg_config": (_lib.MMXPgConfig, ["fit", "clip"])}
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "this test needs a C compiler"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "mmx_api.h"', "int main(void) {", '  printf("{\\"pad\\": 0");']
    for st, (_, names) in members.items():
        lines.append(f'  printf(", \\"{st}\\": %zu", sizeof({st}));')
        lines += [f'  printf(", \\"{st}.{n}\\": %zu", offsetof({st}, {n}));' for n in names]
    lines += ['  printf("}\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, timeout=120)
    got = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout)
    for st, (mirror, names) in members.items():
        assert C.sizeof(mirror) == got[st], st
        assert [f[0].rstrip("_") for f in mirror._fields_] == names
        for f, n in zip(mirror._fields_, names):
            assert getattr(mirror, f[0]).offset == got[f"{st}.{n}"], (st, n)
    hdr = open(os.path.join(REPO, "mujoco_manip_amd", "csrc", "mmx_pg.h")).read()
    assert "#define PG_NORM_EPS 1e-8f" in hdr and R.NORM_EPS == 1e-8
    # NULL arguments are refused without a device
    assert L.mmx_gae(None, None, 1, 1, None, None, None, None, None, None) == -1
    assert L.mmx_policy_fit_pg(None, None, None, None, None, 1, 1, None, None) == -1
    assert L.mmx_policy_set_log_std(None, None) == -1
