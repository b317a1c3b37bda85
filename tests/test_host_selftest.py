"""The library's host-only code under AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU.

csrc/mmx_seed.h (numpy's SeedSequence / PCG64 initialisation restated) and csrc/mmx_plan.h (the rollout's
launch plan and its MMX_PLAN parser) use no HIP.  tests/host/mmx_host_selftest.cpp includes both, is built
here with g++ and the sanitizers, and runs as a child process; any sanitizer finding aborts it.  What it
prints is checked against numpy and against the plan's rules (mmx_plan.h's head comment).
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from rollout_plan_ref import plan_launches

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "mmx_host_selftest.cpp")
SEEDS = (0, 42, 2**40 + 3, 2**64 - 1)
SPAWNS = ((42, 64), (2**40 + 3, 8))
CASES = ((0, 3, 32, 0), (1, 3, 32, 0), (2, 3, 32, 0), (20, 4, 32, 0), (43, 1, 7, 0), (43, 3, 32, 0), (512, 3, 32, 0),
         (43, 3, 32, 1))
# MMX_PLAN strings for a 20-step rollout on 4 lanes: the first is valid, every other falls back
OVERRIDE = "3,4,13;5,5,5,5"
FALLBACK = ("3,4,12;5,5,5,5,5", "", ";", "x", ",,", "5,", "0,20", "-3,23", "2147483647,2147483647")

_OUT = {}


def _run(tmp_path_factory):
    """The program's output lines (parsed), built and run once for the module."""
    if "lines" not in _OUT:
        assert shutil.which("g++"), "this test needs g++ (the sanitizer build of the host self-test)"
        exe = str(tmp_path_factory.mktemp("host_selftest") / "mmx_host_selftest")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], check=True, capture_output=True, timeout=300)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                   UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        r = subprocess.run([exe] + [f"20={p}" for p in (OVERRIDE,) + FALLBACK], capture_output=True, text=True,
                           timeout=120, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        _OUT["lines"] = [json.loads(x) for x in r.stdout.splitlines()]
    return _OUT["lines"]


@pytest.fixture
def lines(tmp_path_factory):
    return _run(tmp_path_factory)


def test_pcg64_seeding_matches_numpy(lines):
    got = {x["seed"]: x for x in lines if x["kind"] == "pcg64"}
    assert set(got) == set(SEEDS)
    for s in SEEDS:
        st = np.random.PCG64(np.random.SeedSequence(s)).state["state"]
        assert (got[s]["state"][0] << 64) | got[s]["state"][1] == st["state"], s
        assert (got[s]["inc"][0] << 64) | got[s]["inc"][1] == st["inc"], s


def test_episode_seeds_match_numpy_spawn(lines):
    got = {(x["root"], x["index"]): x["value"] for x in lines if x["kind"] == "spawn"}
    assert len(got) == sum(n for _, n in SPAWNS)
    for root, n in SPAWNS:
        children = np.random.SeedSequence(root).spawn(n)
        for i in range(n):
            assert got[(root, i)] == int(children[i].generate_state(1)[0]), (root, i)


def test_default_plans(lines):
    plans = {(x["n"], x["lanes"], x["fuse"], x["cameras"]): x for x in lines if x["kind"] == "plan" and x["arg"] < 0}
    assert set(plans) == set(CASES)
    for (n, lanes, fuse, cameras), p in plans.items():
        L = 1 if cameras or n <= 1 else lanes
        assert len(p["len"]) == L, p
        assert p["rounds"] == max(len(v) for v in p["len"])
        if cameras:
            continue
        ln = max(1, min(fuse, -(-n // 4)))
        for l, v in enumerate(p["len"]):
            assert sum(v) == n and all(0 < k <= ln for k in v), p
            first = min(n, l * ln // lanes)
            if first:
                assert v[0] == first, p
            elif n:
                assert v[0] == min(n, ln), p
            # after the lane's first launch: whole launches, then one remainder
            assert all(k == ln for k in v[1:-1]), p
        # the lanes the library uses for n steps make the launches tests/test_gpu.py expects of the sim
        assert p["rounds"] == plan_launches(n, fuse, L), p
    # the pinned 43-step plan on three lanes (test_fused_rollout_bit_identical)
    assert plans[(43, 3, 32, 0)]["len"] == [[11, 11, 11, 10], [3, 11, 11, 11, 7], [7, 11, 11, 11, 3]]
    assert plans[(43, 3, 32, 1)]["len"] == [[1] * 43]  # with cameras: one lane of n ones
    assert plans[(1, 3, 32, 0)]["len"] == [[1]]  # a single step: one lane
    assert plans[(0, 3, 32, 0)]["len"] == [[]] and plans[(0, 3, 32, 0)]["rounds"] == 0


def test_mmx_plan_override_and_fallback(lines):
    by_arg = {x["arg"]: x for x in lines if x["kind"] == "plan" and x["arg"] >= 0}
    assert len(by_arg) == 1 + len(FALLBACK)
    default = next(x for x in lines if x["kind"] == "plan" and x["arg"] < 0 and (x["n"], x["lanes"]) == (20, 4))
    assert default["len"] == [[5, 5, 5, 5], [1, 5, 5, 5, 4], [2, 5, 5, 5, 3], [3, 5, 5, 5, 2]]  # len 5, firsts 0 1 2 3
    # lanes 0 and 1 as written, the last list again for lanes 2 and 3
    assert by_arg[0]["len"] == [[3, 4, 13], [5, 5, 5, 5], [5, 5, 5, 5], [5, 5, 5, 5]] and by_arg[0]["rounds"] == 4
    for k, text in enumerate(FALLBACK, 1):
        assert by_arg[k]["len"] == default["len"] and by_arg[k]["rounds"] == default["rounds"], text
