"""The closed forms of the policy's training step (csrc/mmx_policy_fit.h: the code the kernels run) on the host,
under AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU, and the Python layer's validation.

tests/host/mmx_policy_fit_selftest.cpp is built here with g++ and the sanitizers and run as a child process; nothing
is loaded into python under a sanitizer.  Checked: the fp64 restatement of tests/policy_fit_ref.py against
torch.autograd and torch.optim in float64; the scalar reference step against that restatement (one SGD step at
lr = 1, so the weight change is the gradient) within the gate the GPU test uses, with the padding and everything
outside the layers untouched; Adam's update bit for bit; the batch indices."""
import json
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import policy_fit_ref as R
from policy_ref import make_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "mmx_policy_fit_selftest.cpp")
_EXE = {}
F32 = np.float32


def run(tmp_path_factory, *args):
    if "exe" not in _EXE:
        assert shutil.which("g++"), "this test needs g++ (the sanitizer build of the host program)"
        exe = str(tmp_path_factory.mktemp("policy_fit_host") / "mmx_policy_fit_selftest")
        # -ffp-contract=off: the optimisers' operation order is stated one rounding at a time
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], check=True, capture_output=True, timeout=300)
        _EXE["exe"] = exe
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([_EXE["exe"]] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return [json.loads(x) for x in r.stdout.splitlines()]


def words(a):
    return " ".join(str(int(v)) for v in np.ascontiguousarray(a, F32).view(np.uint32).ravel())


def f32(w):
    return np.array(w, np.uint32).view(F32)


def write_case(path, spec, obs, target, B, shuffle=0, seed=0, k=0, optimizer=0, lr=1.0, b1=0.9, b2=0.999, eps=1e-8, t=1):
    with open(path, "w") as f:
        f.write(f"{len(spec['layers'])} {('tanh', 'relu').index(spec['activation'])} {B} {len(obs)} {shuffle} {seed} {k} {optimizer} "
                f"{words([lr, b1, b2, eps])} {t}\n")
        f.write(" ".join(str(W.shape[0]) for W, _ in spec["layers"]) + "\n")
        for W, b in spec["layers"]:
            f.write(f"{int(b is not None)}\n{words(W)}\n" + (words(b) + "\n" if b is not None else ""))
        for arr in (spec["obs_shift"], spec["obs_scale"], obs, target):
            f.write(words(arr) + "\n")


# ------------------------------------------------------------------ the fp64 restatement against torch
@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_fp64_restatement_against_torch(activation, optimizer):
    torch = pytest.importorskip("torch")
    nn = torch.nn
    spec, obs, target = R.make_case((33, 20), 4, activation, True, 50)
    spec["obs_scale"][17] = 1.0  # torch has no dropped entry; keep the input finite instead
    obs[:, 17] = 0.5
    net64 = R.Net(spec, False)
    act = nn.Tanh if activation == "tanh" else nn.ReLU
    tnet = nn.Sequential(nn.Linear(85, 33), act(), nn.Linear(33, 20), act(), nn.Linear(20, 4)).double()
    with torch.no_grad():
        for m, (W, b) in zip(list(tnet)[0::2], net64.layers):
            m.weight.copy_(torch.from_numpy(W))
            m.bias.copy_(torch.from_numpy(b))
    lr = float(F32(0.01))
    opt = (torch.optim.Adam(tnet.parameters(), lr=lr, eps=float(F32(1e-8)), betas=(float(F32(0.9)), float(F32(0.999))))
           if optimizer == "adam" else torch.optim.SGD(tnet.parameters(), lr=lr))
    x = torch.from_numpy((obs.astype(np.float64) - net64.shift) * net64.scale)
    y = torch.from_numpy(target.astype(np.float64))
    worst = 0.0
    for step in range(5):
        idx = R.batch_indices(1, 9, step, 24, len(obs))
        opt.zero_grad()
        loss = torch.mean((tnet(x[idx]) - y[idx]) ** 2)
        loss.backward()
        _, grads = net64.gradients(obs[idx], target[idx])
        for m, (dW, db) in zip(list(tnet)[0::2], grads):
            worst = max(worst, R.err(dW, m.weight.grad.numpy()), R.err(db, m.bias.grad.numpy()))
        opt.step()
        got = net64.step(obs[idx], target[idx], optimizer, lr=0.01)
        worst = max(worst, abs(got - loss.item()) / loss.item())
        for m, (W, b) in zip(list(tnet)[0::2], net64.layers):
            worst = max(worst, R.err(W, m.weight.detach().numpy()), R.err(b, m.bias.detach().numpy()))
    print("fp64 restatement against torch, worst relative difference:", worst)
    assert worst <= 1e-12


# ------------------------------------------------------------------ the scalar reference step
@pytest.mark.parametrize("B,n", [(1, 3), (63, 70), (65, 65), (65, 20)])
@pytest.mark.parametrize("hidden,A,activation,bias", R.GRAD_CASES)
def test_scalar_step_against_fp64(tmp_path_factory, hidden, A, activation, bias, B, n):
    spec, obs, target = R.make_case(hidden, A, activation, bias, n)
    path = str(tmp_path_factory.mktemp("fit_case") / "case.txt")
    write_case(path, spec, obs, target, B)
    (x,) = run(tmp_path_factory, "step", path)
    idx = R.batch_indices(0, 0, 0, B, n)
    assert (n >= B) or len(set(idx)) < B  # n < B: pairs repeat
    n64, n32 = R.Net(spec, False), R.Net(spec, True)
    loss64 = n64.step(obs[idx], target[idx], "sgd", lr=1.0)
    loss32 = n32.step(obs[idx], target[idx], "sgd", lr=1.0)
    before = R.Net(spec, False).layers
    assert x["pad_nonzero"] == 0 and x["outside_changed"] == 0
    worst = 0.0
    for l, (lay, (W0, b0), (W64, b64), (W32, b32)) in enumerate(zip(x["layers"], before, n64.layers, n32.layers)):
        gotW, gotb = f32(lay["W"]).reshape(W0.shape), f32(lay["b"])
        for got, w0, w64, w32 in ((gotW, W0, W64, W32), (gotb, b0, b64, b32)):
            # the weight change is the gradient (lr = 1); the rounding of w - g itself is charged to the yardstick too
            e_ref, e_yard = R.err(got.astype(np.float64) - w0, w64 - w0), R.err(w32.astype(np.float64) - w0, w64 - w0)
            worst = max(worst, e_ref / (8 * max(e_yard, R.U)))
            assert e_ref <= 8 * max(e_yard, R.U), (l, e_ref, e_yard)
        if l == 0:  # the dropped observation entry: a gradient of exactly 0
            assert (gotW[:, 17] == W0[:, 17].astype(F32)).all()
    e_loss = abs(float(f32([x["loss"]])[0]) - loss64) / loss64
    assert e_loss <= 8 * max(abs(float(loss32) - loss64) / loss64, R.U)
    print("scalar reference: worst fraction of the gate:", worst)


def test_adam_update_bit_for_bit(tmp_path_factory):
    g = [0.0, 1e-30, -1e-12, 3e-5, -0.7, 12.0]
    grid = [(w, gg, m, v, t) for w in (0.3, -1e-3) for gg in g for m, v in ((0.0, 0.0), (1e-4, 1e-38), (-0.2, 0.05)) for t in (1, 2, 1000)]
    args = []
    for w, gg, m, v, t in grid:
        args += words([w, gg, m, v]).split() + [str(t)] + words([1e-3, 0.9, 0.999, 1e-8]).split()
    lines = run(tmp_path_factory, "adam", *args)
    assert len(lines) == len(grid)
    for (w, gg, m, v, t), x in zip(grid, lines):
        ww, mm, vv = R.adam32(F32(w), F32(gg), F32(m), F32(v), t, 1e-3, 0.9, 0.999, 1e-8)
        want = np.array([ww, mm, vv], F32).view(np.uint32)
        assert [x["w"], x["m"], x["v"]] == [int(u) for u in want], (w, gg, m, v, t)
    # g = 0 from a zero state leaves the weight alone; the first step of a fresh state moves it by about lr
    w1, _, _ = R.adam32(F32(0.3), F32(0.0), F32(0), F32(0), 1, 1e-3, 0.9, 0.999, 1e-8)
    w2, _, _ = R.adam32(F32(0.3), F32(-0.7), F32(0), F32(0), 1, 1e-3, 0.9, 0.999, 1e-8)
    assert w1 == F32(0.3) and abs(float(w2) - 0.301) < 1e-6


@pytest.mark.parametrize("n", [1, 2, 130, 2**31 - 1])
def test_batch_indices(tmp_path_factory, n):
    for shuffle, seed, k, B in ((0, 0, 0, 7), (0, 0, 5, 64), (0, 3, 2**33 + 1, 9), (1, 0, 0, 7), (1, 2**63 + 11, 3, 70), (1, 5, 2**32 + 2, 9)):
        (x,) = run(tmp_path_factory, "index", shuffle, seed, k, B, n)
        got = np.array(x["index"], np.int64)
        assert (got == R.batch_indices(shuffle, seed, k, B, n)).all() and got.min() >= 0 and got.max() < n
    (a,), (b,) = run(tmp_path_factory, "index", 1, 4, 1, 64, n), run(tmp_path_factory, "index", 1, 4, 1, 16, n)
    assert a["index"][:16] == b["index"]  # a function of (seed, k, s) alone
    if n > 100:
        (c,) = run(tmp_path_factory, "index", 1, 4, 2, 64, n)
        assert c["index"] != a["index"] and len(set(a["index"])) > 32


# ------------------------------------------------------------------ the Python layer, without a GPU
class _Untouched:
    """Stands where the device object would: any call into the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name})")


def test_fit_validation():
    torch = pytest.importorskip("torch")
    from mujoco_manip_amd import _lib
    from mujoco_manip_amd.policy import MlpPolicy

    spec = make_spec(4, hidden=(16,))
    p = MlpPolicy(spec["layers"])
    obs, tgt = torch.zeros(8, 85), torch.zeros(8, 4)
    with pytest.raises(RuntimeError, match="not bound"):
        p.fit(obs, tgt, 1)
    for call in (p.weights, lambda: p.load(spec["layers"]), lambda: p.to_torch(None)):
        with pytest.raises(RuntimeError, match="not bound"):
            call()
    # bound to a stand-in on the CPU device: every rejection comes before the library is touched
    p._dev, p._env = _Untouched(), types.SimpleNamespace(device="cpu")
    bad = [dict(obs=obs.double()), dict(obs=torch.zeros(8, 84)), dict(target=torch.zeros(8, 5)), dict(target=torch.zeros(7, 4)),
           dict(obs=torch.zeros(85, 8).t()), dict(obs=np.zeros((8, 85), np.float32)), dict(obs=torch.zeros(0, 85), target=torch.zeros(0, 4)),
           dict(steps=-1), dict(optimizer="lbfgs"), dict(batch=0), dict(batch=_lib.FIT_MAX_BATCH + 1), dict(lr=0.0), dict(lr=float("nan")),
           dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1))]
    for kw in bad:
        args = dict(obs=obs, target=tgt, steps=1)
        args.update(kw)
        with pytest.raises(ValueError):
            p.fit(**args)
    p._env = types.SimpleNamespace(device="meta")  # tensors on another device than the policy's
    with pytest.raises(ValueError, match="must be on"):
        p.fit(obs, tgt, 1)
    p._dev = p._env = None
    assert _lib.FIT_OPTIMIZERS == ("sgd", "adam") and _lib.MMXFitConfig().batch == 0


# ------------------------------------------------------------------ the C-ABI boundary
def test_fit_abi_matches_the_header(tmp_path):
    """The three entry points are declared, exported and bound; mmx_fit_config's ctypes mirror has the header's size
    and member offsets (read from a tiny C program); the constants agree with the binding and the kernels' header."""
    import ctypes as C
    import re

    from mujoco_manip_amd import _lib

    api = open(os.path.join(REPO, "include", "mmx_api.h")).read()
    L = _lib.load()
    for sym in ("mmx_policy_fit", "mmx_policy_get_weights", "mmx_policy_set_weights"):
        assert re.search(rf"^int\s+{sym}\s*\(", api, re.M) and hasattr(L, sym) and sym in _lib.EXPORTED, sym
    names = [f[0] for f in _lib.MMXFitConfig._fields_]
    assert names == ["optimizer", "batch", "shuffle", "reset_optimizer", "lr", "beta1", "beta2", "eps", "seed"]
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "this test needs a C compiler"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "mmx_api.h"', "int main(void) {",
             '  printf("{\\"size\\": %zu, \\"sgd\\": %d, \\"adam\\": %d, \\"max_batch\\": %d", sizeof(mmx_fit_config), MMX_FIT_SGD, MMX_FIT_ADAM,',
             "         MMX_FIT_MAX_BATCH);"]
    lines += [f'  printf(", \\"{n}\\": %zu", offsetof(mmx_fit_config, {n}));' for n in names]
    lines += ['  printf("}\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, timeout=120)
    got = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout)
    assert C.sizeof(_lib.MMXFitConfig) == got["size"]
    for n in names:
        assert getattr(_lib.MMXFitConfig, n).offset == got[n], n
    assert _lib.FIT_OPTIMIZERS.index("sgd") == got["sgd"] and _lib.FIT_OPTIMIZERS.index("adam") == got["adam"]
    assert _lib.FIT_MAX_BATCH == got["max_batch"] == 65536
    hdr = open(os.path.join(REPO, "mujoco_manip_amd", "csrc", "mmx_policy_fit.h")).read()
    for text in ("#define FIT_SGD 0 ", "#define FIT_ADAM 1 ", "#define FIT_MAX_BATCH 65536 ", "#define FIT_DOMAIN 0xF17BA7C4u"):
        assert text in hdr, text
    assert R.FIT_DOMAIN == 0xF17BA7C4
    # NULL arguments are refused without a device
    assert L.mmx_policy_fit(None, None, None, 1, 1, None, None) == -1
    assert L.mmx_policy_get_weights(None, None, None) == -1 and L.mmx_policy_set_weights(None, None, None) == -1
