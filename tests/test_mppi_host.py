"""The MPPI planner's closed forms (csrc/mmx_mppi.h: the code the kernels run) on the host, under
AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU.

tests/host/mmx_mppi_selftest.cpp is built here with g++ and the sanitizers and run as a child process; nothing
is loaded into python under a sanitizer.  Checked against the restatements of tests/mppi_ref.py (fp64, written
from the header's text): the Philox4x32-10 known answers, the draw of a grid of (seed, call, t, i, a) (uniforms
exactly, normals within 1e-6: host libm), and mppi_return and the group update for K in {2, 8, 65, 256}: ties
under temperature 0, done flags at t = 0, in the middle and at H - 1, one non-finite return (excluded), a whole
group non-finite (nominal unchanged), gamma < 1.

Bounds of the update (fp32 against fp64): returns within H^2 2^-24 max|r| (step t's fused multiply-add rounds a
sum of at most (t + 1) max|r| by 2^-24 relative, and gamma^t carries t - 1 roundings: together at most
sum_t 2 t 2^-24 max|r| <= H^2 2^-24 max|r|; at H = 3 this is within the H 2^-23 max|r| of the GPU test);
weights within 2e-5 absolute and the new nominal within 2e-5 (high - low): the exponent's argument stays below
50 in magnitude, so its fp32 rounding moves a weight by at most 3e-6 relative, then a 1-2 ulp exponential and
K <= 256 summands.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import mppi_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "mmx_mppi_selftest.cpp")
KAT = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
# seed, call, t, i, a: both halves of seed and call, every a % 4 and a / 4, large i, the last step
GRID = [(s, c, t, i, a) for s in (0, 7, 2**63 + 12345) for c in (0, 1, 2**32 + 5) for t in (0, 3, 63)
        for i in (0, 1, 4095, 2**31 - 1) for a in (0, 1, 2, 3, 4, 7, 9)]
LOW, HIGH = np.array([-0.5, 0.0, 0.24, 0.0]), np.array([0.5, 0.8, 0.60, 1.0])
_EXE = {}


def run(tmp_path_factory, *args):
    if "exe" not in _EXE:
        assert shutil.which("g++"), "this test needs g++ (the sanitizer build of the host program)"
        exe = str(tmp_path_factory.mktemp("mppi_host") / "mmx_mppi_selftest")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], check=True, capture_output=True, timeout=300)
        _EXE["exe"] = exe
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([_EXE["exe"]] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return [json.loads(x) for x in r.stdout.splitlines()]


def test_philox_known_answers(tmp_path_factory):
    lines = run(tmp_path_factory, "philox")
    assert len(lines) == 3
    for x, (ctr, key, want) in zip(lines, KAT):
        want = tuple(int(w, 16) for w in want.split())
        assert tuple(x["out"]) == want
        assert mppi_ref.philox4x32_10(ctr, key) == want  # the restatement the other tests lean on


def test_draw_matches_the_restatement(tmp_path_factory):
    lines = run(tmp_path_factory, "draw", *[v for g in GRID for v in g])
    assert len(lines) == len(GRID)
    worst = 0.0
    for x, (s, c, t, i, a) in zip(lines, GRID):
        assert (x["seed"], x["call"], x["t"], x["i"], x["a"]) == (s, c, t, i, a)
        u1, u2, z = mppi_ref.draw(s, c, t, i, a)
        assert x["u1"] == u1 and x["u2"] == u2, x
        assert 0.0 < u1 <= 1.0 and 0.0 <= u2 < 1.0
        worst = max(worst, abs(x["z"] - z))
    print("normals: max |host - fp64| =", worst)
    assert worst <= 1e-6
    # the element depends on (seed, call, t, i, a) alone, and the four components of a block differ
    zs = {g: x["z"] for g, x in zip(GRID, lines)}
    assert len({zs[(7, 1, 3, 1, a)] for a in (0, 1, 2, 3, 4, 7, 9)}) == 7


def tie_candidates(K):
    return (K // 2 if K > 2 else 0), K - 1


def case(K, temperature, gamma, seed, H=5, M=4, A=4):
    """A case's inputs: M - 1 ordinary groups and a last group whose returns are all non-finite.  Every case
    is real at K = 2 too: the three done flags sit on three candidates of two groups, the tie is candidates
    0 and 1."""
    rng = np.random.default_rng(seed)
    N = M * K
    nominal = rng.uniform(LOW, HIGH, (H, M, A)).astype(np.float32)
    actions = rng.uniform(LOW, HIGH, (H, N, A)).astype(np.float32)
    reward = rng.uniform(0.0, 1.0, (H, N)).astype(np.float32)
    done = np.zeros((H, N, 3), np.int32)
    # group 0: done at t = 0 (terminated) and in the middle (truncated); group 2: done at H - 1
    done[0, 0, 0] = 1
    done[H // 2, 1, 1] = 1
    done[H - 1, 2 * K, 0] = 1
    done[1, 2 * K + 1, 2] = 1  # success alone ends nothing
    # group 1: two equal best candidates (a tie: the lower k must win), and one excluded candidate before them
    lo, hi = tie_candidates(K)
    reward[:, K + hi] = reward[:, K + lo] = 1.0
    done[:, K + hi] = done[:, K + lo] = 0
    if K > 2:
        reward[0, K] = np.nan  # candidate 0 of group 1 is excluded
        reward[3, K + 1] = np.inf
        done[2, K + 1, 1] = 1  # ... but a non-finite reward after the episode's end never reaches the return
    # last group: every return non-finite
    reward[1, (M - 1) * K:] = np.where(np.arange(K) % 2, np.nan, -np.inf)
    return dict(H=H, M=M, K=K, A=A, temperature=temperature, gamma=gamma, nominal=nominal, actions=actions, reward=reward,
                done=done)


def run_case(tmp_path_factory, c):
    path = str(tmp_path_factory.mktemp("mppi_case") / "case.txt")
    box = np.zeros((3, 10), np.float32)
    box[1, :4], box[2, :4] = LOW, HIGH
    with open(path, "w") as f:
        f.write(f"{c['H']} {c['M']} {c['K']} {c['A']} {c['temperature']!r} {c['gamma']!r}\n")
        for arr in (box, c["nominal"], c["actions"], c["reward"]):
            f.write(" ".join(repr(float(v)) for v in arr.ravel()) + "\n")
        f.write(" ".join(str(int(v)) for v in c["done"].ravel()) + "\n")
    (x,) = run(tmp_path_factory, "update", path)
    f32 = lambda name, shape: np.array(x[name], np.uint32).view(np.float32).reshape(shape)  # noqa: E731
    N = c["M"] * c["K"]
    return dict(returns=f32("returns", N), weights=f32("weights", N), finite=f32("finite", N) > 0,
                nominal=f32("nominal", (c["H"], c["M"], c["A"])), action_out=f32("action_out", (c["M"], c["A"])),
                best=np.array(x["best"]))


@pytest.mark.parametrize("K", (2, 8, 65, 256))
@pytest.mark.parametrize("temperature,gamma", ((0.1, 1.0), (0.1, 0.9), (0.0, 0.9)))
def test_return_and_group_update(tmp_path_factory, K, temperature, gamma):
    c = case(K, temperature, gamma, seed=K)
    got = run_case(tmp_path_factory, c)
    want = mppi_ref.update(c["reward"], c["done"], c["actions"], c["nominal"], K, temperature, gamma)
    H, M = c["H"], c["M"]
    fin = np.isfinite(want["returns"])
    assert (got["finite"] == fin).all()
    assert not fin[(M - 1) * K:].any() and fin[:K].all()
    if K > 2:
        assert not fin[K] and fin[K + 1]  # the excluded candidate; the non-finite reward behind the episode's end
    err = np.abs(got["returns"][fin] - want["returns"][fin]).max()
    print("returns: max error", err, "bound", H * H * 2.0 ** -24)
    assert err <= H * H * 2.0 ** -24 * 1.0  # max |r| = 1
    assert (got["best"] == want["best"]).all() and got["best"][M - 1] == -1
    assert got["best"][1] == tie_candidates(K)[0]  # the tie went to the lower k (past the excluded candidate 0)
    assert want["returns"][K + tie_candidates(K)[0]] == want["returns"][2 * K - 1] == want["returns"][K:2 * K][fin[K:2 * K]].max()
    werr = np.abs(got["weights"] - want["weights"]).max()
    print("weights: max error", werr)
    assert werr <= 2e-5
    assert (got["weights"][~fin] == 0).all()
    sums = got["weights"].reshape(M, K).sum(axis=1, dtype=np.float64)
    assert np.abs(sums[:M - 1] - 1.0).max() <= 2e-5 and sums[M - 1] == 0
    if temperature == 0:
        onehot = np.zeros((M, K), np.float32)
        onehot[np.arange(M - 1), got["best"][:M - 1]] = 1
        assert (got["weights"].reshape(M, K) == onehot).all()
    nerr = (np.abs(got["nominal"] - want["nominal"]) / (HIGH - LOW)).max()
    oerr = (np.abs(got["action_out"] - want["action_out"]) / (HIGH - LOW)).max()
    print("nominal, action_out: max error / (high - low)", nerr, oerr)
    assert nerr <= 2e-5 and oerr <= 2e-5
    # the wholly excluded group: its nominal is left as it was, bit for bit, and the output is its first step
    assert (got["nominal"][:, M - 1].view(np.uint32) == c["nominal"][:, M - 1].view(np.uint32)).all()
    assert (got["action_out"][M - 1] == c["nominal"][0, M - 1]).all()
    # the shift: the last step is repeated
    assert (got["nominal"][H - 1, :M - 1] == got["nominal"][H - 2, :M - 1]).all()


def test_nothing_after_the_end_counts(tmp_path_factory):
    """Changing the reward behind an episode's end changes no return."""
    c = case(8, 0.1, 0.9, seed=3)
    a = run_case(tmp_path_factory, c)
    d = dict(c, reward=c["reward"].copy())
    d["reward"][1:, 0] += 5.0  # candidate 0 of group 0 terminated at t = 0
    d["reward"][c["H"] // 2 + 1:, 1] -= 3.0  # candidate 1: truncated in the middle
    b = run_case(tmp_path_factory, d)
    assert (a["returns"].view(np.uint32) == b["returns"].view(np.uint32)).all()
    assert a["returns"][0] == c["reward"][0, 0]
