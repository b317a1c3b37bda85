"""The constraint solver on a ladder of row layouts (tests/solver_row_scenes.py), one env per scene.

Why: from its second iteration on the Newton solver only ever updates its gradient incrementally, group
by group over the stored rows; the loops over the rows run in slices of 64 (RPL = 5 slices), and rows past
MMX_LDSEFC (128 or 192, the two step layouts) are read from the env's HBM overflow block instead of LDS.  A
group missed at a slice or address-space boundary gives a wrong solution that the solver itself reports as
converged.  The states along an expert episode never put a row type's first or last group on such a
boundary on purpose; the scenes here do (test_ladder_premises lists what their union covers).

Checks, on the kernel (`-m gpu`), per layout, one Sim holding all scenes, physics_step without IK:
* no env error, no solver exit above tolerance, the oracle's contact pairs / ncon / nefc after one substep;
* qpos / qvel within the project's L1 bounds (1e-5 / 5e-3 after 1 substep, 1e-4 / 2e-2 after 16);
* after one substep qacc_warmstart against the oracle's qacc, per block (arm dofs, cube dofs).
  integrate_wave leaves E.x, the solver's solution, untouched ("E.x stays: it is the next solve's warm
  start") and store_env writes it to qacc_warmstart, so this compares the solver's solution itself, not
  the velocity it produced through h = 0.002.  The bound is not a fixed number: per scene and block it is
  QACC_FACTOR x the oracle's own spread under one-ulp fp32 perturbations of every qpos and qvel entry
  (16 seeded draws; a draw that changes the contact count is left out, at most 2 of 16).  Why 32: the
  spread models one rounding of the inputs; the kernel also rounds a 9-joint kinematic chain, contact
  geometry at 0.5 m, Jacobian rows and impedances.  The bound must stay below 5e-3 / h = 2.5, the L1
  bound on the same quantity;
* the two layouts bit-identical on qpos, qvel, qacc_warmstart and the contact record;
* the oracle's relative residual at the kernel's solution (or_eval_cost), recorded only: the fp32 problem
  differs from the fp64 one.

On the CPU: the premises, and a mutation check: a numpy restatement of the solver whose gradient leaves
out the rows stored at 192 and above, or the last group of a row type, converges to a solution that breaks
the qacc bound (so the bound would catch such a miss).

Out of reach: rows 257..320.  Every scene keeps ncon <= 60 (the record holds 64), and 60 contacts with the
largest possible single block (the equality and nine limits: 12 rows) are 252 stored rows; the fifth row
slice (rows 257..320) needs 62 contacts or more, which no pose found here gives below the contact cap.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cube_contact_scenes as S  # noqa: E402
import solver_row_scenes as R  # noqa: E402

torch = pytest.importorskip("torch")

H_STEP = 0.002
QACC_FACTOR = 32.0
NDRAW = 16
ROWS = [128, 192]
ARM, CUBES = slice(0, 9), slice(9, 27)
BLOCKS = (("arm", ARM), ("cubes", CUBES))

_REF = {}


def _oracle(state):
    return S.oracle_env([np.asarray(a, np.float64) for a in state])


def _ulp_draw(state, rng):
    """Every qpos and qvel entry one fp32 ulp up or down."""
    q, v, c, w = state
    out = []
    for a in (q, v):
        up = rng.integers(0, 2, a.shape).astype(bool)
        out.append(np.where(up, np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))).astype(np.float32))
    return out[0], out[1], c, w


def _reference():
    """Per scene, from the fp32 states the kernel runs (once, shared, never modified): the layout, the
    oracle's contacts / nefc / qacc / Newton iterations of the first substep, its states after 1 and 16
    substeps, and the input-rounding spread of qacc per block."""
    if "ref" in _REF:
        return _REF["ref"]
    out = []
    for k, (name, st) in enumerate(R.scenes()):
        e = _oracle(st)
        lay = R.row_layout(e)
        _, i0 = e.solver_stats()
        e.mj_forward()
        iters = e.solver_stats()[1] - i0
        cons = S.oracle_contacts(e)
        d = dict(name=name, layout=lay, iters=iters, pairs=sorted((c[0], c[1]) for c in cons), ncon=len(cons), nefc=e.nefc(),
                 dists=[c[2] for c in cons], qacc=e.qacc().copy(), resid=e.solver_residual(), env=e)
        e2 = _oracle(st)
        states = {}
        for n in range(1, 17):
            e2.mj_step()
            if n in (1, 16):
                states[n] = e2.get_state()[:2]
        d["after"] = states
        rng = np.random.default_rng(1000 + k)
        spread = {b: 0.0 for b, _ in BLOCKS}
        used = 0
        for _ in range(NDRAW):
            ep = _oracle(_ulp_draw(st, rng))
            if len(ep.contacts()) != d["ncon"]:
                continue
            used += 1
            for b, sl in BLOCKS:
                spread[b] = max(spread[b], float(np.abs(ep.qacc()[sl] - d["qacc"][sl]).max()))
        d["spread"], d["draws_used"] = spread, used
        out.append(d)
    _REF["ref"] = out
    return out


def _bound(d, block):
    return QACC_FACTOR * d["spread"][block]


# --------------------------------------------------------------------------- CPU: premises
def _straddles(lay, t, L):
    a, b = R.contact_rows(lay, t)
    return a < L < b


def test_ladder_premises():
    """The union of the scenes reaches every class of layout at which the solver's loops have an edge."""
    ref = _reference()
    lays = [d["layout"] for d in ref]
    types = [(lay, t) for lay in lays for t in range(R.NTYPE) if lay["count"][t]]
    covered = {}
    covered["every type non-empty"] = all(any(lay["count"][t] for lay in lays) for t in range(R.NTYPE))
    covered["a type of one group"] = any(lay["count"][t] == 1 for lay, t in types)
    covered["odd and even group counts"] = {lay["count"][t] % 2 for lay, t in types} == {0, 1}
    for L in (128, 192):
        side = {(L - R.contact_rows(lay, t)[0]) // 4 % 2 for lay, t in types if _straddles(lay, t, L)}
        covered[f"straddles {L}: odd and even LDS-side group counts"] = side == {0, 1}
        covered[f"a type begins or ends at {L}"] = any(L in R.contact_rows(lay, t) for lay, t in types)
    for r in (64, 128, 192):
        covered[f"a type crosses row {r}"] = any(_straddles(lay, t, r) for lay, t in types)
    totals = [lay["total"] for lay in lays]
    for lo, hi in ((0, 64), (65, 128), (129, 192), (193, 256)):
        covered[f"a total in {lo}..{hi}"] = any(lo <= n <= hi for n in totals)
    covered["a total that is a multiple of 64"] = any(n % 64 == 0 for n in totals)
    covered["nsingle 4 and 8"] = {lay["nsingle"] for lay in lays} >= {4, 8}
    covered["two scenes of 200 rows or more"] = sum(n >= 200 for n in totals) >= 2
    covered["two arm-cube types at once"] = any(sum(lay["count"][t] > 0 for t in (1, 2, 3)) >= 2 for lay in lays)
    covered["type 0 with contacts beside cube contacts"] = any(lay["count"][0] and sum(lay["count"][4:]) for lay in lays)
    covered["ncon <= 60 everywhere"] = all(lay["ncon"] <= 60 for lay in lays)
    covered["no contact within 1e-5 m of the margin"] = all(x < -1e-5 for d in ref for x in d["dists"])
    covered["two Newton iterations or more above 128 rows"] = all(d["iters"] >= 2 for d in ref if d["layout"]["total"] > 128)
    covered["the oracle converged"] = all(d["resid"] < 1e-12 for d in ref)
    for d in ref:
        print(f"{d['name']:24s} rows {d['layout']['total']:3d} ncon {d['ncon']:2d} nsingle {d['layout']['nsingle']} "
              f"tbase {d['layout']['tbase']} newton {d['iters']}")
    for k, v in covered.items():
        print(("covered      " if v else "NOT COVERED  ") + k)
    assert all(covered.values()), [k for k, v in covered.items() if not v]
    assert max(totals) <= 256  # the fifth row slice stays out of reach (module docstring)


def test_qacc_bounds_from_the_oracles_spread(margin):
    """The per-scene bounds: at most 2 of 16 draws changed the contact count, every spread is positive, and
    32 x spread stays below the L1 bound on the same quantity, 5e-3 / h."""
    for d in _reference():
        assert d["draws_used"] >= NDRAW - 2, (d["name"], d["draws_used"])
        for b, _ in BLOCKS:
            margin(f"{d['name']}_{b}_qacc_bound", _bound(d, b), 5e-3 / H_STEP, spread=d["spread"][b], draws=d["draws_used"])
            assert 0.0 < _bound(d, b) < 5e-3 / H_STEP, (d["name"], b, d["spread"][b])


# --------------------------------------------------------------------------- CPU: mutation check
def _contact_groups(d):
    """Per contact of the oracle env (in its order): (row type, first stored row of its group, its MuJoCo
    rows in the oracle's row order).  A type's contacts keep the contact order; the oracle's rows are the
    equality, the limits, then each contact's pyramid edges."""
    e, lay = d["env"], d["layout"]
    rows = e.efc()
    first = int((rows["type"] != 2).sum())
    assert (rows["type"][first:] == 2).all()
    nedge = (len(rows["type"]) - first) // d["ncon"] if d["ncon"] else 0
    assert first + nedge * d["ncon"] == len(rows["type"])  # every contact here has the same number of edges
    seen = [0] * R.NTYPE
    out = []
    for c, (g1, g2) in enumerate((c[0], c[1]) for c in S.oracle_contacts(e)):
        t = R.contact_type(g1, g2)
        out.append((t, R.contact_rows(lay, t)[0] + 4 * seen[t], list(range(first + nedge * c, first + nedge * (c + 1)))))
        seen[t] += 1
    return out


def _np_solve(d, drop=()):
    """Primal Newton on the oracle's rows, restated in numpy: cost 1/2 (x - a0)' M (x - a0) + sum of
    1/2 D r^2 over the active rows (r = J x - aref; equality always, others when r < 0), started from the
    warm start, full Hessian of the active set.  The rows in `drop` are left out of the GRADIENT only (the
    kernel's incremental gradient update missing a group); the iteration then converges to where that
    gradient vanishes.  Steps are halved until the gradient norm decreases."""
    e = d["env"]
    J, rows, M = e.efc_J(), e.efc(), e.mass_matrix()
    D, aref, eq = 1.0 / rows["R"], rows["aref"], rows["type"] == 0
    a0 = e.smooth()["qacc_smooth"]
    keep = np.ones(len(D))
    keep[list(drop)] = 0.0

    def grad(x):
        r = J @ x - aref
        act = eq | (r < 0)
        return M @ (x - a0) + J.T @ (D * r * act * keep), act

    x = a0.copy()
    g, act = grad(x)
    for _ in range(200):
        if np.linalg.norm(g) < 1e-9:
            break
        Hm = M + (J.T * (D * act)) @ J
        p = -np.linalg.solve(Hm, g)
        alpha = 1.0
        while alpha > 1e-6:
            g2, act2 = grad(x + alpha * p)
            if np.linalg.norm(g2) < np.linalg.norm(g):
                break
            alpha *= 0.5
        x, g, act = x + alpha * p, g2, act2
    return x, float(np.linalg.norm(g))


def test_missed_groups_break_the_qacc_bound(margin):
    """The numpy restatement reproduces the oracle's solution.  With rows left out of its gradient, its
    solution is further from the oracle's than the qacc bound in some block:
    * the rows stored at L and above, for L = 128 in every scene above 128 rows and for L = 192 in every scene
      with two groups or more there (the whole overflow side of a layout missed);
    * the last group of a row type, for at least one type of every scene above 128 rows; every type's
      figure is recorded.  What the bound does NOT catch is one missed group of a redundant contact set: a
      cube pressed into a bin corner rests on 12 face corners, and without one of them its acceleration
      moves by 0.3 to 0.9 of the bound (the other corners of the face take the load)."""
    ref = _reference()
    tested = 0
    for d in ref:
        lay = d["layout"]
        if lay["total"] <= 128:
            continue
        x, gn = _np_solve(d)
        assert gn < 1e-6 and np.abs(x - d["qacc"]).max() < 1e-6, (d["name"], gn, np.abs(x - d["qacc"]).max())
        groups = _contact_groups(d)

        def ratio(drop):
            xm, _ = _np_solve(d, drop)
            return max(float(np.abs(xm[sl] - d["qacc"][sl]).max()) / _bound(d, b) for b, sl in BLOCKS)

        for L in (128, 192):
            past = [rr for _, base, rr in groups if base >= L]
            if len(past) >= 2:
                w = ratio([r for rr in past for r in rr])
                margin(f"{d['name']}_rows_from_{L}_error_over_bound", w, None, groups_dropped=len(past))
                assert w > 1.0, (d["name"], L, w)
                tested += 1
        single = {}
        for t in range(R.NTYPE):
            mine = [g for g in groups if g[0] == t]
            if mine:
                single[t] = ratio(max(mine, key=lambda g: g[1])[2])
                margin(f"{d['name']}_last_group_of_type_{t}_error_over_bound", single[t], None, groups=len(mine))
        assert max(single.values()) > 1.0, (d["name"], single)
        tested += 1
    assert tested >= 20


# --------------------------------------------------------------------------- GPU (HIP kernel)
_GPU = {}


def _gpu_run(rows, nsub):
    from mujoco_manip_amd import _lib

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    if (rows, nsub) not in _GPU:
        _lib.load(build_if_missing=False)
        scenes = R.scenes()
        sim = _lib.Sim(len(scenes), action_mode="abs_pos", image_size=0)
        sim.reset()
        sim.step_rows = rows
        assert sim.step_rows == rows
        sim.set_state(*[np.stack([st[k] for _, st in scenes]) for k in range(4)])
        sim.physics_step(nsub, with_ik=False)
        q, v, _, w = sim.get_state()
        epi = sim.view("episode_i", _lib.EPI_N, "<i4").cpu().numpy().copy()
        ncon = epi[:, _lib.EPI["ncon"]]
        assert (ncon < _lib.MAXCON).all(), ncon
        raw = sim.view("contacts", _lib.MAXCON * _lib.CON_F).cpu().numpy().reshape(-1, _lib.MAXCON, _lib.CON_F).copy()
        for e in range(len(scenes)):
            raw[e, ncon[e]:] = 0.0  # entries past ncon are not part of the record
        cols = [_lib.STAT_FIELDS.index(k) for k in ("sum_solver_iter", "exit_stall", "exit_cap")]
        solve = sim.view("stats", _lib.STAT_N).cpu().numpy()[:, cols].astype(float)
        sim.close()
        _GPU[(rows, nsub)] = dict(q=q, v=v, w=w, ncon=ncon.copy(), nefc=epi[:, _lib.EPI["nefc"]].copy(),
                                  err=epi[:, _lib.EPI["env_error"]].copy(), raw=raw, solve=solve)
    return _GPU[(rows, nsub)]


@pytest.mark.gpu
@pytest.mark.parametrize("nsub,tol_q,tol_v", [(1, 1e-5, 5e-3), (16, 1e-4, 2e-2)], ids=["substep1", "substep16"])
@pytest.mark.parametrize("rows", ROWS)
def test_gpu_ladder_parity(rows, nsub, tol_q, tol_v, margin):
    """L1 parity on the ladder: no env error, no solver exit above tolerance, the oracle's contacts after
    the first substep, qpos / qvel within the project's bounds."""
    ref = _reference()
    g = _gpu_run(rows, nsub)
    assert (g["err"] == 0).all(), g["err"]
    first = _gpu_run(rows, 1)
    bad = []
    for k, d in enumerate(ref):
        pairs = sorted((int(c[11]), int(c[12])) for c in first["raw"][k, :first["ncon"][k]])
        assert (first["ncon"][k], first["nefc"][k]) == (d["ncon"], d["nefc"]), (d["name"], first["ncon"][k], first["nefc"][k])
        assert pairs == d["pairs"], d["name"]
        dq = float(np.abs(g["q"][k] - d["after"][nsub][0]).max())
        dv = float(np.abs(g["v"][k] - d["after"][nsub][1]).max())
        margin(f"{d['name']}_max_abs_dqpos", dq, tol_q)
        margin(f"{d['name']}_max_abs_dqvel", dv, tol_v)
        margin(f"{d['name']}_newton_iterations_per_substep", float(g["solve"][k, 0]) / nsub, None, oracle_first_substep=d["iters"],
               exits_above_tolerance=float(g["solve"][k, 1:].sum()))
        print(f"{d['name']:24s} rows {d['layout']['total']:3d} dqpos {dq:.2e} dqvel {dv:.2e} newton {g['solve'][k, 0] / nsub:.1f}")
        if not (dq < tol_q and dv < tol_v):
            bad.append((d["name"], dq, dv))
    assert (g["solve"][:, 0] >= nsub).all(), g["solve"][:, 0]  # Newton iterations are recorded
    assert g["solve"][:, 1:].sum() == 0, g["solve"]  # exit_stall, exit_cap
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS)
def test_gpu_ladder_solution(rows, margin):
    """After one substep qacc_warmstart (the solver's solution) against the oracle's qacc, per block, within
    32 x the oracle's input-rounding spread of that scene; the oracle's residual at the kernel's solution
    is recorded."""
    ref = _reference()
    g = _gpu_run(rows, 1)
    assert (g["err"] == 0).all(), g["err"]
    bad = []
    for k, d in enumerate(ref):
        _, _, resid = d["env"].eval_cost(g["w"][k].astype(float))
        margin(f"{d['name']}_oracle_residual_at_kernel_solution", resid, None, oracle_own=d["resid"])
        for b, sl in BLOCKS:
            err = float(np.abs(g["w"][k][sl] - d["qacc"][sl]).max())
            margin(f"{d['name']}_{b}_max_abs_dqacc", err, _bound(d, b), spread=d["spread"][b])
            print(f"{d['name']:24s} {b:5s} dqacc {err:.3e} bound {_bound(d, b):.3e} spread {d['spread'][b]:.3e} resid {resid:.1e}")
            if not err < _bound(d, b):
                bad.append((d["name"], b, err, _bound(d, b)))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("nsub", [1, 16])
def test_gpu_ladder_layouts_agree(nsub, margin):
    """The 128-row and the 192-row kernel (with its helper wave) are bit-identical on the whole ladder: qpos,
    qvel, qacc_warmstart and the contact record."""
    a, b = _gpu_run(128, nsub), _gpu_run(192, nsub)
    margin("max_abs_dstate", max(float(np.abs(a[k] - b[k]).max()) for k in ("q", "v", "w")), 0.0)
    for k in ("q", "v", "w", "ncon", "nefc", "raw"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
