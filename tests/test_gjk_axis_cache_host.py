"""The axis cache's verdict and slot policy (csrc/mmx_gjk_cache.h: the code the step kernels run) on the host,
under AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU.

tests/host/mmx_gjk_cache_selftest.cpp is built here with g++ and the sanitizers and run as a child process;
nothing is loaded into python under a sanitizer.

The verdict (gjkc_separated) must refuse an empty (zero) entry, a stale one (a direction along which the pair
is no longer separated), another pair's entry and every non-finite or over-long direction, whatever the support
difference is, and accept a true separating axis only beyond the margin m: the cases straddle m by one part in
a thousand, far outside the rounding of the three products (2^-22 relative).  The slot policy (gjkc_slot) must
stay inside the table for every hit / busy mask and pair index, return the pair's own slot when it has one, and
never a slot another pair of the same pass holds.
"""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "mmx_gjk_cache_selftest.cpp")
_EXE = {}


def run(tmp_path_factory, *args, stdin=""):
    if "exe" not in _EXE:
        assert shutil.which("g++"), "this test needs g++ (the sanitizer build of the host program)"
        exe = str(tmp_path_factory.mktemp("gjk_cache_host") / "mmx_gjk_cache_selftest")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], check=True, capture_output=True, timeout=300)
        _EXE["exe"] = exe
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([_EXE["exe"]] + [str(a) for a in args], input=stdin, capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def verdicts(tmp_path_factory, cases):
    """cases: (tag, pair, d (3 floats or 3 ints = raw bits), w (3 floats)) -> list of bool."""
    lines = []
    for tag, pair, d, w in cases:
        words = [x if isinstance(x, int) else bits(x) for x in d] + [x if isinstance(x, int) else bits(x) for x in w]
        lines.append(f"{tag} {pair} " + " ".join(f"{x:x}" for x in words))
    out = run(tmp_path_factory, "verdict", stdin="\n".join(lines) + "\n")
    assert len(out) == len(cases)
    return [x == "1" for x in out]


def constants(tmp_path_factory):
    (line,) = run(tmp_path_factory, "constants")
    return json.loads(line)


def test_margin_is_what_the_derivation_asks(tmp_path_factory):
    c = constants(tmp_path_factory)
    # at least 8 x the 1e-6 m rounding bound of w . d, and under the sweep's smallest near-miss gap
    assert 8e-6 <= c["margin"] < 4e-5
    assert c["words"] == 4 and 1 <= c["slots"] <= 32


def test_verdict_refuses_what_proves_nothing(tmp_path_factory):
    m = constants(tmp_path_factory)["margin"]
    rng = np.random.default_rng(5)
    unit = rng.normal(size=(40, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    INF, NINF, NAN, SNAN = 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001
    deep = (-0.3, -0.2, -0.1)  # w for which every direction below "separates" if it were trusted
    cases, want = [], []
    # an empty entry: zero tag and zero direction, for pair 0 too (whose tag is 1)
    for pair in (0, 1, 779):
        cases.append((0, pair, (0.0, 0.0, 0.0), deep)), want.append(False)
    cases.append((1, 0, (0.0, 0.0, 0.0), deep)), want.append(False)  # the right tag, the zero direction
    cases.append((1, 0, (-0.0, -0.0, -0.0), deep)), want.append(False)
    for u in unit:
        d = tuple(float(np.float32(x)) for x in u)
        far = tuple(float(np.float32(-0.05 * x)) for x in u)   # 5 cm beyond the pair along d
        near = tuple(float(np.float32(+0.05 * x)) for x in u)  # the pair has since closed past the axis: stale
        cases.append((8, 7, d, far)), want.append(True)
        cases.append((8, 7, d, near)), want.append(False)            # stale
        cases.append((8, 7, d, (0.0, 0.0, 0.0))), want.append(False)  # touching
        cases.append((9, 7, d, far)), want.append(False)             # another pair's entry
        cases.append((7, 7, d, far)), want.append(False)             # the pair index itself is not its tag
        cases.append((0, 7, d, far)), want.append(False)
        # beyond the margin, and just inside it
        cases.append((8, 7, d, tuple(float(np.float32(-1.001 * m * x)) for x in u))), want.append(True)
        cases.append((8, 7, d, tuple(float(np.float32(-0.999 * m * x)) for x in u))), want.append(False)
        # an over-long direction makes m no metric margin: refused, however far apart the pair is
        cases.append((8, 7, tuple(float(np.float32(1.01 * x)) for x in u), far)), want.append(False)
        cases.append((8, 7, tuple(float(np.float32(3.0 * x)) for x in u), far)), want.append(False)
    # non-finite words in every component, with finite and with non-finite support differences
    for bad in (INF, NINF, NAN, SNAN, 0xFFFFFFFF, bits(1e30), bits(-1e30), bits(2.0)):
        for k in range(3):
            d = [bits(0.0)] * 3
            d[k] = bad
            cases.append((8, 7, tuple(d), deep)), want.append(False)
            d = [bits(-0.5)] * 3
            d[k] = bad
            cases.append((8, 7, tuple(d), (0.3, 0.2, 0.1))), want.append(False)
    # a sound direction against a non-finite support difference (a diverged env)
    for bad in (INF, NINF, NAN):
        for k in range(3):
            w = [bits(-0.3)] * 3
            w[k] = bad
            cases.append((8, 7, (0.6, 0.0, 0.8), tuple(w))), want.append(False)
    got = verdicts(tmp_path_factory, cases)
    wrong = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not wrong, wrong[:5]


def test_slot_policy_stays_inside_the_table(tmp_path_factory):
    n_slots = constants(tmp_path_factory)["slots"]
    allm = (1 << n_slots) - 1
    lines = [json.loads(x) for x in run(tmp_path_factory, "slots", 11, 20000)]
    assert len(lines) == 20000
    seen = set()
    for x in lines:
        s, hit, busy = x["slot"], x["hit"] & allm, x["busy"] & allm
        assert -1 <= s < n_slots, x
        if hit:
            assert s == (hit & -hit).bit_length() - 1, x  # the pair's own entry, the lowest
        elif busy == allm:
            assert s == -1, x  # every slot held by a pair of this pass: the pair stays uncached
        else:
            assert s >= 0 and not (busy >> s) & 1, x  # never a slot another pair of the pass holds
            first = next(k for k in range(n_slots) if not (busy >> ((x["pair"] % (2 ** 32) % n_slots + k) % n_slots)) & 1)
            assert s == (x["pair"] % (2 ** 32) % n_slots + first) % n_slots, x
        seen.add(s)
    assert seen == set(range(-1, n_slots))
