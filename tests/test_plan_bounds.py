"""The bounds of the time-budgeted step launches (csrc/mmx_plan.h rollout_bounds) under AddressSanitizer +
UndefinedBehaviorSanitizer, without a GPU.

tests/host/mmx_plan_bounds_selftest.cpp is built here with g++ and the sanitizers and run as a child process.
The program itself checks, for every n in 1..600, lanes in 1..8 and fuse in 1..32 and every lane of the plan:
lo_j <= c_j <= hi_j (c_j = the fixed plan's count after launch j), both sequences non-decreasing and within
[0, n], hi_j - lo_j <= len, the first launch fixed, lo_K = hi_K = n, short calls (fewer than 6 launches: all of
fewer than 4, and the driver's 20-step windows) entirely fixed, and everything fixed with the switch off; a
violated rule is its exit status 1.  What it prints is checked here: rollout_plan's lengths against the plan's
rule restated below (a digest over n = 1..600 for every lane count and four fuse caps: the plan is what it was;
tests/test_host_selftest.py pins single plans), and the bounds of a few cases against the rule restated below
and against pinned values.
"""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "mmx_plan_bounds_selftest.cpp")
# n, lanes, fuse: C3's 512-step window, the driver's 20-step window, the GPU tests' shapes, odd ones
CASES = ((512, 4, 32), (20, 4, 32), (24, 2, 4), (48, 2, 4), (43, 3, 32), (600, 8, 7), (1, 4, 32), (15, 3, 32), (16, 1, 32))
# MMX_PLAN strings for 20 steps on 4 lanes: launches of very unequal lengths
OVERRIDES = ("1,1,1,1,1,1,14", "14,1,1,1,1,1,1;5,5,5,5", "1,18,1", "2,2,2,2,2,2,2,2,2,2")

_OUT = {}


def plan(n, lanes, fuse):
    """rollout_plan without cameras (mmx_plan.h's head comment): the lanes' launch lengths."""
    L = lanes if n > 1 else 1
    ln = max(1, min(fuse, -(-n // 4)))
    out = []
    for l in range(L):
        first = min(n, l * ln // lanes)
        v = [first] if first else []
        rem = n - first
        while rem > 0:
            v.append(min(rem, ln))
            rem -= v[-1]
        out.append(v)
    return out, ln


def bounds(v, ln):
    """rollout_bounds: spread len / 2, 0 at the first and the last launch, halving over the last three before
    it, changing by at most a launch's length per launch; fixed below 6 launches."""
    K, n = len(v), sum(v)
    s = [0] * K
    if K >= 6:
        for j in range(1, K - 1):
            d = K - 1 - j
            s[j] = min(ln // 2 if d >= 3 else (ln // 2) >> (3 - d), s[j - 1] + v[j])
        for j in range(K - 2, -1, -1):
            s[j] = min(s[j], s[j + 1] + v[j + 1])
    c = [sum(v[:j + 1]) for j in range(K)]
    return [max(0, c[j] - s[j]) for j in range(K)], [min(n, c[j] + s[j]) for j in range(K)]


def fnv(h, v):
    return ((h ^ (v & 0xFFFFFFFF)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF


DIGEST_FUSE = (4, 7, 16, 32)  # (restating every cap in Python would take a minute)


@pytest.fixture
def lines(tmp_path_factory):
    """The program's output lines (parsed), built and run once for the module."""
    if "lines" not in _OUT:
        assert shutil.which("g++"), "this test needs g++ (the sanitizer build of the host program)"
        exe = str(tmp_path_factory.mktemp("plan_bounds") / "mmx_plan_bounds_selftest")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], check=True, capture_output=True, timeout=300)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                   UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        args = ["%d,%d,%d" % c for c in CASES] + [f"20,4,32={p}" for p in OVERRIDES]
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        _OUT["lines"] = [json.loads(x) for x in r.stdout.splitlines()]
    return _OUT["lines"]


def test_rules_hold_and_the_plan_is_unchanged(lines):
    """Exit status 0 = every rule held in every case (the fixture); the plan's lengths are the restated rule's."""
    dig = {(x["lanes"], x["fuse"]): x for x in lines if x["kind"] == "digest"}
    assert set(dig) == {(l, f) for l in range(1, 9) for f in range(1, 33)}
    for (lanes, fuse), x in dig.items():
        if fuse not in DIGEST_FUSE:
            continue
        h = 1469598103934665603
        for n in range(1, 601):
            p, _ = plan(n, lanes, fuse)
            h = fnv(h, len(p))
            for v in p:
                h = fnv(h, -1)
                for k in v:
                    h = fnv(h, k)
        assert x["plan"] == "%016x" % h, (lanes, fuse)
    # the budget applies somewhere (long calls) and not everywhere (short ones)
    # (one-step launches have no spread to give)
    assert dig[(4, 32)]["budgeted"] > 0 and dig[(2, 4)]["budgeted"] > 0 and dig[(1, 1)]["budgeted"] == 0
    assert all(x["budgeted"] < x["lanes"] * 600 for x in dig.values())


def test_bounds_of_cases(lines):
    got = {(x["n"], x["lanes"], x["fuse"], x["lane"]): x for x in lines if x["kind"] == "bounds"}
    for n, lanes, fuse in CASES:
        p, ln = plan(n, lanes, fuse)
        for l, v in enumerate(p):
            x = got[(n, lanes, fuse, l)]
            assert x["len"] == v, x
            assert (x["lo"], x["hi"]) == bounds(v, ln), x
    # C3's 512-step window, lane 0: sixteen 32-step launches, +-16 in the middle, +-8, +-4, then all at 512
    x = got[(512, 4, 32, 0)]
    assert x["lo"][:3] == [32, 48, 80] and x["hi"][:3] == [32, 80, 112]
    assert x["lo"][-4:] == [400, 440, 476, 512] and x["hi"][-4:] == [432, 456, 484, 512]
    # lane 1 starts with its 8-step offset, fixed
    x = got[(512, 4, 32, 1)]
    assert x["len"][:2] == [8, 32] and (x["lo"][:2], x["hi"][:2]) == ([8, 24], [8, 56])
    # short calls, fixed: the driver's 20-step window (4 or 5 launches of 5 per lane), fewer than 4 launches
    for key in ((20, 4, 32, 0), (20, 4, 32, 1), (20, 4, 32, 2), (20, 4, 32, 3), (1, 4, 32, 0), (15, 3, 32, 0), (16, 1, 32, 0)):
        x = got[key]
        assert x["lo"] == x["hi"], x


def test_bounds_under_plan_overrides(lines):
    """Unequal launch lengths (MMX_PLAN): the program's rules held (the fixture); the spread follows the rule."""
    got = [x for x in lines if x["kind"] == "override"]
    assert len(got) == 4 * len(OVERRIDES)
    for x in got:
        assert sum(x["len"]) == 20
        assert (x["lo"], x["hi"]) == bounds(x["len"], 5), x
    first = got[0]
    assert first["len"] == [1, 1, 1, 1, 1, 1, 14]
    assert first["lo"] == [1, 1, 1, 2, 4, 6, 20] and first["hi"] == [1, 3, 5, 6, 6, 6, 20]
