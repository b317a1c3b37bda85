"""Build libmmx.so (HIP kernels + C-ABI) in-tree for gfx950 with hipcc.

Two variants share the sources: ``libmmx.so`` (the product) and ``libmmx_prof.so``, the same
code compiled with ``-DMMX_PHASE_CLOCK`` so the kernels add per-phase shader-clock cycles into
the stats buffer (selected at load time with ``MMX_PROFILE=1``; never used by the bench).
"""
from __future__ import annotations

import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libmmx.so")
LIB_PROF = os.path.join(PKG, "libmmx_prof.so")
SOURCES = ["mmx_kernels.hip", "mmx_step_l192.hip", "mmx_render.hip", "mmx_render_lit.hip", "mmx_png.hip",
           "mmx_snapshot.hip", "mmx_mppi.hip", "mmx_policy.hip", "mmx_policy_fit.hip", "mmx_api.cpp"]
ARCH = os.environ.get("MMX_OFFLOAD_ARCH", "gfx950")
# device-code math: x / y as x * rcp(y) and sqrt without the denormal-scaling wrapper (v_rcp_f32 /
# v_sqrt_f32, <= 1 ulp) instead of the correctly rounded fdiv / sqrt expansions (~10 VALU each).
# The env-step kernel is VALU-issue-bound at 8 envs per CU: -11 % VALU instructions in the substep,
# +3.7 % env steps/s (C3), parity tolerances unchanged.  Host code keeps IEEE semantics.
# r04: no NaN / Inf / signed-zero semantics either (-ffinite-math-only -fno-signed-zeros): selects
# and min / max lose their NaN guards, -2.3 % VALU instructions per env step and +1.1 % env steps/s
# in the interleaved A/B (profiles/archive/r04_ab_finite_math.json), GPU suite unchanged.  The divergence
# detector (NaN / Inf / |v| >= 1e10 -> counted reset) is an integer bit test, exact under any of these.
DEVICE_MATH = ["-Xarch_device", "-freciprocal-math", "-Xarch_device", "-fapprox-func",
               "-Xarch_device", "-ffinite-math-only", "-Xarch_device", "-fno-signed-zeros"]
# gfx950 machine scheduler: the iterative ILP strategy (schedules for latency within the 256-VGPR
# budget the 2-waves-per-SIMD occupancy allows) measured +6.4 % env steps/s over the default
# occupancy-driven scheduler on the C3 bench (max-ilp +2 %, max-memory-clause +0 %).  The option
# is an LLVM backend flag; the host compile accepts and ignores it.
DEVICE_SCHED = ["-mllvm", "-amdgpu-sched-strategy=" + os.environ.get("MMX_SCHED", "iterative-ilp")]
if os.environ.get("MMX_SCHED") == "default":  # experiments: the backend's default scheduler
    DEVICE_SCHED = []
# no SLP vectorisation in device code: at -O3 it packs pairs of independent fp32 ops into
# v_pk_fma_f32 / v_pk_mul_f32 on even-aligned register pairs (2,700 packed ops in the substep); the
# pairing constraints raised the substep's register pressure into scratch spills (frame 480 -> 172 B)
# and the packed ops bought no issue slots: C3 1.905M -> 2.100M env steps/s in the A/B
DEVICE_NOSLP = ["-Xarch_device", "-fno-slp-vectorize"]
# extra compiler flags (experiments only; the committed build uses none)
FLAGS = DEVICE_MATH + DEVICE_SCHED + DEVICE_NOSLP + os.environ.get("MMX_EXTRA_FLAGS", "").split()
# per-source flags.  The env-step kernel (r04 end): floating-point reassociation in device code
# (-fassociative-math; explicit fmaf / DPP / readlane reductions keep their written order), -2 %
# VALU instructions per env step, C3 +0.9 % in the interleaved A/B (profiles/archive/r04_ab_assoc.json),
# GPU suite unchanged.  Not the renderer, whose shared-edge functions rely on one evaluation order.
# The planner's kernels keep NaN / Inf semantics (the later flag wins over DEVICE_MATH's): their test for a
# non-finite return is plain C++ on the bits of a value the compiler saw computed, and under
# -ffinite-math-only it folds to "finite" (the step kernel hides its values behind an opaque register copy
# instead; these kernels use no inline assembly).  Same registers, no scratch; they are no hot path.
# The policy's training step keeps IEEE division and square root: Adam's update is stated operation by operation
# (csrc/mmx_policy_fit.h) and the device computes it as the host does.
SOURCE_FLAGS = {"mmx_kernels.hip": ["-Xarch_device", "-fassociative-math"],
                "mmx_step_l192.hip": ["-Xarch_device", "-fassociative-math"],
                "mmx_mppi.hip": ["-Xarch_device", "-fno-finite-math-only"],
                "mmx_policy_fit.hip": ["-Xarch_device", "-fno-reciprocal-math", "-Xarch_device", "-fno-approx-func"]}


# test-only builds of the step kernel (tests/test_overflow_kat.py, tests/test_helper_layout.py): both
# step sources (STEP_SOURCES: the 128-row and the 192-row kernel) with defines that force a rare path;
# linked with the product objects of the other sources
STEP_SOURCES = ["mmx_kernels.hip", "mmx_step_l192.hip"]
HIPCC_JOBS = 16  # concurrent hipcc processes of one build()
TEST_VARIANTS = {
    # a 4-entry collision candidate list (product: 320): the sphere-test overflow path, flagged as
    # ERR_CON_OVERFLOW in env_error
    "libmmx_col4.so": ["MMX_COL_LIST=4", "MMX_CAND_CAP=4"],
    # a 1-entry persistent broadphase list: every collision pass runs the full 780-pair prune (the
    # list-vs-full-prune bit-identity test)
    "libmmx_nolist.so": ["MMX_CAND_CAP=1"],
    # the GJK pair class without its cache of separating axes (csrc/mmx_gjk_cache.h): every call runs the whole
    # GJK from its start direction (the cache-on-equals-cache-off test, tests/test_gjk_axis_cache.py), and the
    # product's step kernels with the same counters, probe set 15 (GJK calls, separated calls, support-query
    # rounds, cached verdicts in the stats; no phase clock): the cache is taken, and only where it is compiled in
    "libmmx_nocache.so": ["MMX_GJK_CACHE=0", "MMX_PROBE=15"],
    "libmmx_gjkprobe.so": ["MMX_PROBE=15"],
    # the 192-row kernel with one of its two waves held back after barriers C and A (MMX_HELPER_DELAY in
    # mmx_step_lds.inc: 1 the helper wave, 2 the env wave), and probe set 14 (full prunes and the list's
    # displacement bound in the stats): results may not depend on which wave is late
    "libmmx_hdelay.so": ["MMX_HELPER_DELAY=1", "MMX_PROBE=14"],
    "libmmx_edelay.so": ["MMX_HELPER_DELAY=2", "MMX_PROBE=14"],
    # the budgeted step launches' clock replaced by a cost of 1 + env % 3 "ticks" per env step (MMX_BUDGET_SYNTH in
    # mmx_step_kernels.inc): envs progress unevenly in the same way on every machine (tests/test_step_budget.py)
    "libmmx_synth.so": ["MMX_BUDGET_SYNTH=1"],
}


def lib_path(profile: bool = False) -> str:
    return LIB_PROF if profile else LIB


def test_variant(name: str) -> str:
    """The path of the built test library `name` (a key of TEST_VARIANTS, or libmmx_prof.so), for Sim(lib=...)."""
    path = os.path.join(PKG, name)
    if not os.path.exists(path):
        raise RuntimeError("test build missing: run __graft_entry__.build()")
    return path


def _stale(lib: str) -> bool:
    """Any source-like file of csrc/ (sources, headers, the included step file and its parts) or public header newer than `lib`."""
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    inc = os.path.join(PKG, "..", "include")
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h", ".inc"))]
    deps += [os.path.join(inc, f) for f in os.listdir(inc) if f.endswith(".h")]
    return any(os.path.getmtime(d) > t for d in deps)


def _hipcc(src: str, obj: str, defines: list[str] | tuple = (), profile: bool = False, verbose: bool = False) -> str:
    """Compile csrc/`src` into `obj`: the one place a hipcc compile command is put together (the product and
    profile builds, TEST_VARIANTS and build_variant differ in `defines`, `profile` and the object's path only)."""
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + (["-xhip"] if src.endswith(".cpp") else [])
    cmd += FLAGS + SOURCE_FLAGS.get(src, []) + [f"-D{d}" for d in defines] + (["-DMMX_PHASE_CLOCK=1"] if profile else [])
    cmd += [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, src), "-o", obj]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return obj


def _link(out: str, objs: list[str]) -> str:
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", out] + objs)
    return out


def _obj(src: str, tag: str = "") -> str:
    return os.path.join(CSRC, os.path.splitext(src)[0] + tag + ".o")


def build(force: bool = False, verbose: bool = False, profile: bool | None = False) -> str:
    """Build one variant (profile=False/True) or both (profile=None, which also builds the test-only
    TEST_VARIANTS); returns the product path."""
    variants = [False, True] if profile is None else [profile]
    variants = [v for v in variants if force or _stale(lib_path(v))]
    tests = [n for n in TEST_VARIANTS if profile is None and (force or _stale(os.path.join(PKG, n)))]
    if variants or tests:
        # the profile build's probe set: MMX_PROBE in the environment, 1 by default
        pdef = [f"MMX_PROBE={int(os.environ.get('MMX_PROBE', '1'))}"]
        jobs = [(src, v) for v in variants for src in SOURCES]
        tjobs = [(n, src) for n in tests for src in STEP_SOURCES]
        with ThreadPoolExecutor(max_workers=min(HIPCC_JOBS, len(jobs) + len(tjobs))) as ex:
            tobjs = [ex.submit(_hipcc, src, _obj(src, "_" + os.path.splitext(n)[0]), TEST_VARIANTS[n], False, verbose)
                     for n, src in tjobs]
            objs = list(ex.map(lambda j: _hipcc(j[0], _obj(j[0], "_prof" if j[1] else ""), pdef if j[1] else [], j[1], verbose), jobs))
            tobjs = [f.result() for f in tobjs]
        for v in variants:
            _link(lib_path(v), [o for o, (_, vv) in zip(objs, jobs) if vv == v])
        for n in tests:  # the variant's step kernels + the product's objects of the other sources
            kobjs = [o for o, (nn, _) in zip(tobjs, tjobs) if nn == n]
            _link(os.path.join(PKG, n), kobjs + [_obj(src) for src in SOURCES if src not in STEP_SOURCES])
    return lib_path(bool(profile))


if __name__ == "__main__":
    print(build(force=True, verbose=True, profile=None))


def build_variant(out: str, defines: list[str], profile: bool = True) -> str:
    """Diagnostic / experiment build of the same sources with extra -D defines into `out`
    (e.g. build/libmmx_prof5.so for probe set 5); loaded with MMX_LIB_PATH.  Not the product."""
    tag = os.path.splitext(os.path.basename(out))[0]
    where = os.path.dirname(os.path.abspath(out))
    os.makedirs(where, exist_ok=True)
    with ThreadPoolExecutor(max_workers=len(SOURCES)) as ex:
        objs = list(ex.map(lambda src: _hipcc(src, os.path.join(where, f"{tag}_{os.path.splitext(src)[0]}.o"), defines, profile), SOURCES))
    return _link(out, objs)
