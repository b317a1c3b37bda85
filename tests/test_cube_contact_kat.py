"""Cube-on-cube contact: the coupled Newton solve pinned to closed forms and to the fp64 oracle.

When two cubes touch, the kernel's Newton solver leaves its block Cholesky for the general
arrow-ordered one (chol_solve_arrow: elimination order cube 1, cube 2, cube 3, arm; fill-in
bookkeeping on the coupling mask; its 27 x 27 transpose in the env's HBM overflow block, at an
offset that differs between the 128-row and 192-row layouts), fed by the Hessian tiles of the
three cube-cube row types (pairs (c1, c2), (c1, c3), (c2, c3)).  No expert episode of the C3
workload has two cubes in contact, so the states here are built (tests/cube_contact_scenes.py):

  1. closed forms, derived from MuJoCo's published equations as in tests/test_physics_kat.py and
     extended to two free bodies: a two-cube stack at rest (4 table contacts carry 2 m g at
     t = 20, 8 cube-cube contacts carry m g at t = 20 + 20) and the first substep of a slow push on
     the upper cube (12 dof, 72 active pyramid edges), for the three index pairs;
  2. GPU vs oracle parity (the project's L1 bounds) on two-cube stacks, three-cube stacks with
     each cube in the middle (eliminating the middle block first or last changes the fill-in) and
     a held cube pressed on another (arm-cube and cube-cube coupling, fill-in arm-cube; rows past
     128, so the 128-row layout has overflow rows beside the transpose); both layouts, which must
     agree bit for bit;
  3. dynamic scenes in lockstep with the oracle (edges switching, the Hessian updated
     incrementally): a push on the upper cube, a push from the side, a drop;
  4. one episode of the product path (PickPlaceVecEnv, expert actions) whose release puts the red
     cube on the green one.

The fp64 oracle solves with a dense Cholesky (oracle/or_physics.c), so it shares none of the
kernel's block structure.  Every scene asserts that its cube-cube contacts are there.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cube_contact_scenes as S  # noqa: E402
from collision_geometry import CUBES, quat2mat  # noqa: E402
from test_physics_kat import G, HALF, M_CUBE, TRAN, a_hat_pyramid, impedance, kb, rest_penetration  # noqa: E402

PUSH = 0.02
# Newton iterations allowed where every pyramid edge is active (resting or slowly pushed stacks): the
# cost is then exactly quadratic, so one Newton step with an exact factorisation lands on the
# minimum; fp32 rounding against the relative gradient tolerance (1e-6, ~10 ulp) may take one or two
# refinements.  The result alone would not show a wrong factorisation that Newton's later
# iterations correct (a missed fill-in block, a wrong lane in the transposed solve): the count does.
QUADRATIC_ITER = 3
PAIR_IDS = [f"{CUBES[a]}-{CUBES[b]}" for a, b in S.PAIRS]
ROWS = [128, 192]


def _v12(v, lo, up):
    return np.r_[v[9 + 6 * lo: 15 + 6 * lo], v[9 + 6 * up: 15 + 6 * up]].astype(float)


# --------------------------------------------------------------------------- closed forms (CPU)
def test_stack_rest_closed_form_discriminates_weights():
    """The rest answers (MuJoCo documentation: R = (1 - d) / d * A_hat, A_hat = 2 mu0^2 (t + mu0^2 t),
    t the sum of BOTH bodies' translational invweight0): -0.747438 mm under the stack, -0.509692 mm
    between the cubes; with one body's weight only (t = 20) the cube-cube depth differs by many
    times the GPU tolerance (2e-6)."""
    assert abs(S.P_TABLE_2 - -0.747438e-3) < 1e-9, S.P_TABLE_2
    assert abs(S.P_CUBE - -0.509692e-3) < 1e-9, S.P_CUBE
    one_body = rest_penetration(8, tran=TRAN)
    assert abs(S.P_CUBE - one_body) > 10 * 2e-6, (S.P_CUBE, one_body)
    # the answers carry the loads: edges x D aref = the weight above
    K, _ = kb()
    for ncon, p, tran, load in ((4, S.P_TABLE_2, TRAN, 2 * M_CUBE * G), (8, S.P_CUBE, 2 * TRAN, M_CUBE * G)):
        d = impedance(p)
        assert abs(6 * ncon * K * d * d * -p / ((1 - d) * a_hat_pyramid(tran)) - load) < 1e-9


_SETTLED = {}


def _oracle_settled_stack(lo, up):
    """The oracle's two-cube stack after 1500 substeps from the closed-form rest pose (shared by
    the rest and first-step tests; read only)."""
    if (lo, up) not in _SETTLED:
        e = S.oracle_env(S.stack_state((lo, up)))
        for _ in range(1500):
            e.mj_step()
        _SETTLED[(lo, up)] = (e.get_state(), S.oracle_contacts(e), e.efc())
    return _SETTLED[(lo, up)]


@pytest.mark.parametrize("pair", S.PAIRS, ids=PAIR_IDS)
def test_oracle_stack_rest(pair, margin):
    """The oracle's settled stack sits at the closed-form depths with 4 + 8 contacts, at rest, and
    every cube-cube edge's R is the published formula with t = 40."""
    lo, up = pair
    (q, v, _, _), cons, efc = _oracle_settled_stack(lo, up)
    tab, cc = S.split_contacts(cons, lo, up)
    assert (len(tab), len(cc)) == (4, 8), (len(tab), len(cc))
    zl, zu = S.stack_rest_heights()
    errs = [abs(c[2] - S.P_TABLE_2) for c in tab] + [abs(c[2] - S.P_CUBE) for c in cc]
    errs += [abs(S.cube(q, lo)[0][2] - zl), abs(S.cube(q, up)[0][2] - zu)]
    margin("max_abs_ddepth_dheight", max(errs), 2e-8)
    assert max(errs) < 2e-8, errs
    for o in (lo, up):
        np.testing.assert_allclose(v[9 + 6 * o: 15 + 6 * o], 0.0, atol=1e-9)
    rows = efc["type"] == 2
    assert rows.sum() == 6 * (4 + 8 + 4)  # the stack and the third cube on the table
    # contact rows come in contact order, 6 pyramid edges each (the third cube's table contacts sit
    # at the cube-cube depth: 4 contacts at t = 20 and 8 at t = 40 carry m g alike)
    R = efc["R"][rows].reshape(-1, 6)
    pos = efc["pos"][rows].reshape(-1, 6)
    n_cc = 0
    for i, c in enumerate(cons):
        cube_cube = (c[0], c[1]) == S.pair_geoms(lo, up)
        n_cc += cube_cube
        d = impedance(c[2])
        want = (1 - d) / d * a_hat_pyramid(2 * TRAN if cube_cube else TRAN)
        assert np.abs(pos[i] - c[2]).max() < 1e-12 and np.abs(R[i] - want).max() < 1e-9 * want, (i, c[:3], R[i], want)
    assert n_cc == 8


def _first_step_inputs(q, cons, lo, up):
    com = [S.cube(q, o)[0].astype(float) for o in (lo, up)]
    rot = [quat2mat(S.cube(q, o)[1].astype(float)) for o in (lo, up)]
    tab, cc = S.split_contacts(cons, lo, up)
    assert (len(tab), len(cc)) == (4, 8), (len(tab), len(cc))
    return com, rot, tab, cc


@pytest.mark.parametrize("pair", S.PAIRS, ids=PAIR_IDS)
def test_oracle_stack_first_step_closed_form(pair, margin):
    """The settled stack's upper cube given 0.02 m/s along x (inside the pyramids: all 72 edges stay
    active): one substep gives the velocity of the 12-dof closed-form primal solution (upper vx
    0.0178800, lower vx 0.00058546: the lower cube is dragged along)."""
    lo, up = pair
    (q, v, c, w), cons, _ = _oracle_settled_stack(lo, up)
    com, rot, tab, cc = _first_step_inputs(q, cons, lo, up)
    v = v.copy()
    v[9 + 6 * up] = PUSH
    e = S.oracle_env((q, v, c, w))
    e.mj_step()
    got = _v12(e.get_state()[1], lo, up)
    want = S.first_step_velocity_2(com, rot, _v12(v, lo, up), tab, cc)
    margin("max_abs_dqvel", float(np.abs(got - want).max()), 1e-9)
    np.testing.assert_allclose(got, want, atol=1e-9)
    assert abs(want[6] - 0.0178800) < 1e-7 and abs(want[0] - 0.00058546) < 1e-8, (want[6], want[0])


def test_first_step_closed_form_discriminates_coupling():
    """The 12-dof answer depends on the cube-cube coupling: solved block-diagonally (the two
    off-diagonal 6 x 6 blocks of the system matrix zeroed, what a solve that missed the coupling
    would do) the lower cube's vx is 1.90e-3 instead of 5.85e-4 and the upper one's 1.674e-2 instead
    of 1.788e-2: 66 and 57 times the GPU tolerance (2e-5)."""
    lo, up = S.PAIRS[0]
    (q, v, c, w), cons, _ = _oracle_settled_stack(lo, up)
    com, rot, tab, cc = _first_step_inputs(q, cons, lo, up)
    v = v.copy()
    v[9 + 6 * up] = PUSH
    want = S.first_step_velocity_2(com, rot, _v12(v, lo, up), tab, cc)
    mut = S.first_step_velocity_2(com, rot, _v12(v, lo, up), tab, cc, couple=False)
    assert abs(mut[0] - want[0]) > 10 * 2e-5, (mut[0], want[0])
    assert abs(mut[6] - want[6]) > 10 * 2e-5, (mut[6], want[6])


# --------------------------------------------------------------------------- scene premises (CPU)
def test_parity_scene_premises():
    """What the coupled parity states hold, on the oracle: the expected cube-cube pairs with 8
    contacts each, before and after 1 and 16 substeps (the cube under a held one: 1; it is pushed
    off after 4 to 12 substeps); two-cube stacks 4 + 8 (+ 4 of the third cube)
    contacts and 97 rows, three-cube stacks 4 + 8 + 8 and 121 rows, a held cube on another 39-44
    contacts and 235-265 rows (so > 128 stored rows: 6 pyramid edges are 4 stored basis rows)."""
    from mujoco_manip_amd import _lib

    scenes = S.parity_scenes()
    assert len(scenes) == 12
    seen_pairs, middles, held = set(), set(), set()
    for name, st, pairs in scenes:
        e = S.oracle_env(st)
        stays = not name.startswith("held")  # the cube under a held one is pushed off within 16 substeps
        for nsub in (0, 1, 15) if stays else (0, 1):
            for _ in range(nsub):
                e.mj_step()
            cons = S.oracle_contacts(e)
            assert len(cons) < _lib.MAXCON, (name, len(cons))
            for p in pairs:
                assert sum(1 for c in cons if (c[0], c[1]) == p) == 8, (name, nsub, p)
            ncc = sum(1 for c in cons if c[0] in S.CUBE_GEOM and c[1] in S.CUBE_GEOM)
            assert ncc == 8 * len(pairs), (name, nsub, ncc)
        e = S.oracle_env(st)
        cons = S.oracle_contacts(e)
        e.mj_step()
        rows = e.nefc()
        kind = name.split(":")[0]
        if kind != "held":  # every pyramid edge pushes: the first solve is a quadratic problem (QUADRATIC_ITER)
            assert (e.efc_force()[e.efc()["type"] == 2] > 0).all(), name
        if kind == "stack2":
            assert (len(cons), rows) == (16, 97), (name, len(cons), rows)
        elif kind == "stack3":
            assert (len(cons), rows) == (20, 121), (name, len(cons), rows)
            middles.add(pairs[0][0] if pairs[0][0] in pairs[1] else pairs[0][1])
        else:
            assert 39 <= len(cons) <= 44 and 235 <= rows <= 265, (name, len(cons), rows)
            assert rows - 2 * len(cons) > 128, (name, rows, len(cons))
            held.add(name)
        seen_pairs.update(pairs)
    assert seen_pairs == {S.pair_geoms(a, b) for a, b in S.PAIRS}
    assert middles == set(S.CUBE_GEOM)  # each cube has been the middle of a chain
    assert len(held) == 6               # each cube held against each other cube


def test_dynamic_scene_premises():
    """The lockstep scenes on the oracle: cube-cube contact in at least half of the substeps; the
    pushed upper cube slides about 18 mm, the dropped cube lands within 20 mm + its penetration."""
    for name, st, n, (a, b) in S.dynamic_scenes():
        e = S.oracle_env(st)
        q0 = e.get_state()[0].copy()
        touch = 0
        for _ in range(n):
            e.mj_step()
            touch += any((c[0], c[1]) == S.pair_geoms(a, b) for c in S.oracle_contacts(e))
        assert 2 * touch >= n, (name, touch, n)
        q = e.get_state()[0]
        if name == "top_push":
            assert 0.015 < S.cube(q, b)[0][0] - S.cube(q0, b)[0][0] < 0.021
        if name == "drop":
            assert abs(S.cube(q, b)[0][2] - S.cube(q0, b)[0][2] + 0.020) < 0.0015


def _oracle_stack_episode():
    """The expert's (red, bin_red) episode from the keyframe with the green cube put, unrotated,
    where red comes to rest in the undisturbed episode: (env steps, env steps with red-green contact,
    final qpos, green's start pose)."""
    import oracle_py as O

    def run(green):
        e = O.OracleEnv(action_mode="abs_pos", reward_type="staged", task=(S.RED, 0))
        e.reset(seed=0)
        if green is not None:
            q, v, c, w = e.get_state()
            S.put(q, S.GREEN, green)
            e.set_state(q, v, c, w)
            e.mj_forward()
        e.fsm_init([(S.RED, 0)])
        n = touch = 0
        for _ in range(500):
            if e.fsm_plan(16) == 10:
                break
            f = e.fsm_get()
            e.step(np.array([*f["target"], float(f["gripper_open"])], np.float32))
            n += 1
            touch += any((c[0], c[1]) == S.pair_geoms(S.RED, S.GREEN) for c in S.oracle_contacts(e))
        return n, touch, e.get_state()[0]

    if "ep" not in _SETTLED:
        _, _, q = run(None)
        green = S.cube(q, S.RED)[0].astype(np.float32).astype(float)
        _SETTLED["ep"] = run(green) + (green,)
    return _SETTLED["ep"]


def test_oracle_stack_episode_premise():
    """The product-path episode on the oracle: the release puts red on green (red's centre one cube
    above green's, inside the bin), with red-green contact over many env steps."""
    n, touch, q, green = _oracle_stack_episode()
    red, grn = S.cube(q, S.RED)[0], S.cube(q, S.GREEN)[0]
    assert n < 200 and touch >= 10, (n, touch)
    assert abs(red[2] - 0.300) < 0.002 and abs(red[2] - grn[2] - 2 * HALF) < 0.002, (red, grn)
    assert np.hypot(*(red[:2] - grn[:2])) < 0.005 and np.linalg.norm(grn - green) < 0.005


# --------------------------------------------------------------------------- GPU (HIP kernel)
def _sim(n, rows):
    from mujoco_manip_amd import _lib

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    _lib.load(build_if_missing=False)
    sim = _lib.Sim(n, action_mode="abs_pos", image_size=0)
    sim.reset()
    sim.step_rows = rows
    assert sim.step_rows == rows
    return sim


def _set(sim, states):
    arrs = [np.stack([np.asarray(s[k], np.float32) for s in states]) for k in range(4)]
    sim.set_state(*arrs)
    return arrs


def _record(sim):
    """Per env: the contacts of the last substep as [(g1, g2, dist, pos, normal)], and the raw record."""
    from mujoco_manip_amd import _lib

    ncon = sim.view("episode_i", _lib.EPI_N, "<i4")[:, _lib.EPI["ncon"]].cpu().numpy().copy()
    raw = sim.view("contacts", _lib.MAXCON * _lib.CON_F).cpu().numpy().reshape(-1, _lib.MAXCON, _lib.CON_F).copy()
    assert (ncon < _lib.MAXCON).all(), ncon
    cons = [[(int(c[11]), int(c[12]), float(c[0]), c[1:4].astype(float), c[4:7].astype(float))
             for c in raw[e, :ncon[e]]] for e in range(len(ncon))]
    for e in range(len(ncon)):
        raw[e, ncon[e]:] = 0.0  # entries past ncon are not part of the record
    return cons, ncon, raw


def _errors(sim):
    from mujoco_manip_amd import _lib

    return sim.view("episode_i", _lib.EPI_N, "<i4")[:, _lib.EPI["env_error"]].cpu().numpy()


def _solver_stats(sim):
    """Per env, summed over the substeps so far: Newton iterations, solves that ended above the
    tolerance on no progress, and at the iteration cap."""
    from mujoco_manip_amd import _lib

    cols = [_lib.STAT_FIELDS.index(k) for k in ("sum_solver_iter", "exit_stall", "exit_cap")]
    return sim.view("stats", _lib.STAT_N).cpu().numpy()[:, cols].astype(float)


_GPU = {}


def _gpu_stack_run(rows):
    """The three two-cube stacks (one env per pair) from the closed-form rest pose: 250 substeps,
    then the push on the upper cubes and one substep more.  Run once per layout, shared."""
    if ("stack", rows) not in _GPU:
        sim = _sim(len(S.PAIRS), rows)
        _set(sim, [S.stack_state(p) for p in S.PAIRS])
        sim.physics_step(250, with_ik=False)
        q, v, c, w = sim.get_state()
        cons, _, _ = _record(sim)
        v1 = v.copy()
        for e, (lo, up) in enumerate(S.PAIRS):
            v1[e, 9 + 6 * lo: 15 + 6 * lo] = 0.0
            v1[e, 9 + 6 * up: 15 + 6 * up] = [PUSH, 0, 0, 0, 0, 0]
        sim.set_state(q, v1, c, w)
        before = _solver_stats(sim)
        sim.physics_step(1, with_ik=False)
        v2 = sim.get_state()[1]
        solve = _solver_stats(sim) - before
        assert (_errors(sim) == 0).all()
        sim.close()
        _GPU[("stack", rows)] = (q, v, cons, v1, v2, solve)
    return _GPU[("stack", rows)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("pair", range(3), ids=PAIR_IDS)
def test_gpu_stack_rest(pair, rows, margin):
    """The kernel's two-cube stack, started at the closed-form rest pose, stays there over 250
    substeps: 4 + 8 contacts at the closed-form depths, both heights, at rest."""
    lo, up = S.PAIRS[pair]
    q, v, cons, _, _, _ = _gpu_stack_run(rows)
    tab, cc = S.split_contacts(cons[pair], lo, up)
    on_pair = [c for c in cons[pair] if {c[0], c[1]} & {S.CUBE_GEOM[lo], S.CUBE_GEOM[up]}]
    assert (len(tab), len(cc), len(on_pair)) == (4, 8, 12), (len(tab), len(cc), len(on_pair))
    zl, zu = S.stack_rest_heights()
    errs = [abs(c[2] - S.P_TABLE_2) for c in tab] + [abs(c[2] - S.P_CUBE) for c in cc]
    errs += [abs(float(S.cube(q[pair], lo)[0][2]) - zl), abs(float(S.cube(q[pair], up)[0][2]) - zu)]
    vmax = float(np.abs(_v12(v[pair], lo, up)).max())
    margin("max_abs_ddepth_dheight", max(errs), 2e-6)
    margin("max_abs_qvel", vmax, 1e-4)
    assert max(errs) < 2e-6, errs
    assert vmax < 1e-4, vmax


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("pair", range(3), ids=PAIR_IDS)
def test_gpu_stack_first_step_closed_form(pair, rows, margin):
    """The push on the upper cube of the kernel's resting stack: one substep against the 12-dof
    closed form evaluated at the contacts the kernel reports."""
    lo, up = S.PAIRS[pair]
    q, _, cons, v1, v2, solve = _gpu_stack_run(rows)
    margin("newton_iterations", float(solve[pair, 0]), None, exit_no_progress=float(solve[pair, 1]),
           exit_iteration_cap=float(solve[pair, 2]))
    com, rot, tab, cc = _first_step_inputs(q[pair], cons[pair], lo, up)
    want = S.first_step_velocity_2(com, rot, _v12(v1[pair], lo, up), tab, cc)
    got = _v12(v2[pair], lo, up)
    margin("max_abs_dqvel", float(np.abs(got - want).max()), 2e-5)
    margin("lower_vx", float(got[0]), None, closed_form=float(want[0]))
    np.testing.assert_allclose(got, want, atol=2e-5)  # 0.1 % of the push
    assert solve[pair, 0] <= QUADRATIC_ITER and solve[pair, 1:].sum() == 0, solve[pair]


_REF = {}


def _parity_ref(nsub):
    """Oracle results of the parity batch from the fp32 states the kernel runs (once, shared)."""
    if "scenes" not in _REF:
        _REF["scenes"] = S.parity_scenes()
    if nsub not in _REF:
        out = []
        for _, st, _ in _REF["scenes"]:
            e = S.oracle_env([np.asarray(a, np.float32).astype(float) for a in st])
            for _ in range(nsub):
                e.mj_step()
            out.append(e.get_state()[:2])
        _REF[nsub] = out
    return _REF["scenes"], _REF[nsub]


def _gpu_parity_run(rows, nsub):
    from mujoco_manip_amd import _lib

    if ("parity", rows, nsub) not in _GPU:
        scenes, _ = _parity_ref(nsub)
        sim = _sim(len(scenes), rows)
        _set(sim, [st for _, st, _ in scenes])
        sim.physics_step(nsub, with_ik=False)
        q, v, _, w = sim.get_state()
        cons, ncon, raw = _record(sim)
        stats = sim.view("stats", _lib.STAT_N)[:, :2].cpu().numpy().copy()
        solve = _solver_stats(sim)
        err = _errors(sim).copy()
        sim.close()
        _GPU[("parity", rows, nsub)] = dict(q=q, v=v, w=w, cons=cons, ncon=ncon, raw=raw, stats=stats, err=err, solve=solve)
    return _GPU[("parity", rows, nsub)]


@pytest.mark.gpu
@pytest.mark.parametrize("nsub,tol_q,tol_v", [(1, 1e-5, 5e-3), (16, 1e-4, 2e-2)], ids=["substep1", "substep16"])
@pytest.mark.parametrize("rows", ROWS)
def test_gpu_coupled_parity(rows, nsub, tol_q, tol_v, margin):
    """L1 parity (fp32 kernel vs fp64 oracle, the project's bounds) on the twelve coupled states.
    Every env's contact record holds its cube-cube pairs, so the general solve ran; the held-cube
    states' stored rows pass 128, so the 128-row layout keeps rows in the overflow block."""
    scenes, ref = _parity_ref(nsub)
    g = _gpu_parity_run(rows, nsub)
    assert (g["err"] == 0).all(), g["err"]
    dq = np.array([np.abs(g["q"][k] - ref[k][0]).max() for k in range(len(scenes))])
    dv = np.array([np.abs(g["v"][k] - ref[k][1]).max() for k in range(len(scenes))])
    # coverage: the record of the first substep (the 16-substep run starts with the same one) holds
    # every scene's cube-cube pairs; the stacks keep them to the end (a cube under a held one is
    # pushed off after 4 to 12 substeps: test_parity_scene_premises)
    first = _gpu_parity_run(rows, 1)
    for k, (name, _, pairs) in enumerate(scenes):
        for p in pairs:
            assert sum((c[0], c[1]) == p for c in first["cons"][k]) == 8, f"{name}: geoms {p} not touching"
            if not name.startswith("held"):
                assert sum((c[0], c[1]) == p for c in g["cons"][k]) == 8, f"{name}: geoms {p} not touching"
    if nsub == 1:
        stored = g["stats"][:, 0] - 2 * g["stats"][:, 1]  # 6 pyramid edges per contact are 4 stored rows
        held = [k for k, (name, _, _) in enumerate(scenes) if name.startswith("held")]
        margin("held_stored_rows_min", float(stored[held].min()))
        assert len(held) == 6 and (stored[held] > 128).all(), stored
    for kind in ("stack2", "stack3", "held"):
        idx = [k for k, (name, _, _) in enumerate(scenes) if name.startswith(kind)]
        margin(f"{kind}_max_abs_dqpos", float(dq[idx].max()), tol_q)
        margin(f"{kind}_max_abs_dqvel", float(dv[idx].max()), tol_v)
        margin(f"{kind}_newton_iterations_per_substep", float(g["solve"][idx, 0].max()) / nsub, None,
               exits_above_tolerance=float(g["solve"][idx, 1:].sum()))
    if nsub == 1:  # the stacks start with every edge active: a quadratic problem (QUADRATIC_ITER)
        stacks = [k for k, (name, _, _) in enumerate(scenes) if name.startswith("stack")]
        assert (g["solve"][stacks, 0] <= QUADRATIC_ITER).all() and g["solve"][stacks, 1:].sum() == 0, g["solve"]
    assert dq.max() < tol_q, dict(zip([s[0] for s in scenes], dq))
    assert dv.max() < tol_v, dict(zip([s[0] for s in scenes], dv))


@pytest.mark.gpu
@pytest.mark.parametrize("nsub", [1, 16])
def test_gpu_coupled_layouts_agree(nsub, margin):
    """The 128-row and 192-row layouts give bit-identical results on the coupled states: qpos, qvel,
    the solver's solution (qacc_warmstart) and the contact record (test_step_layouts_agree's claim,
    extended to the general solve).  physics_step runs the one-substep kernel of the sim's layout
    (mmx_physics_step), so the two runs are the single-wave 128-row kernel and the 192-row kernel
    with its helper wave."""
    a, b = _gpu_parity_run(128, nsub), _gpu_parity_run(192, nsub)
    d = max(float(np.abs(a[k] - b[k]).max()) for k in ("q", "v", "w"))
    margin("max_abs_dstate", d, 0.0)
    np.testing.assert_array_equal(a["q"], b["q"])
    np.testing.assert_array_equal(a["v"], b["v"])
    np.testing.assert_array_equal(a["w"], b["w"])
    np.testing.assert_array_equal(a["ncon"], b["ncon"])
    np.testing.assert_array_equal(a["raw"], b["raw"])


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS)
def test_gpu_dynamic_scenes_follow_oracle(rows, margin):
    """A push on the upper cube (it slides 18 mm and lifts), a push from the side and a drop, each
    in lockstep with the oracle started from the same fp32 state: the cube poses stay within 1 mm
    (quaternion components within 1e-3) at every substep, with cube-cube contact in the kernel's
    record in at least half of the substeps."""
    scenes = S.dynamic_scenes()
    sim = _sim(len(scenes), rows)
    arrs = _set(sim, [st for _, st, _, _ in scenes])
    refs = [S.oracle_env([a[k].astype(float) for a in arrs]) for k in range(len(scenes))]
    worst = np.zeros(len(scenes))
    touch = np.zeros(len(scenes), int)
    for t in range(max(n for _, _, n, _ in scenes)):
        sim.physics_step(1, with_ik=False)
        gq = sim.get_state()[0]
        cons, _, _ = _record(sim)
        for k, (name, _, n, (a, b)) in enumerate(scenes):
            if t >= n:
                continue
            refs[k].mj_step()
            worst[k] = max(worst[k], float(np.abs(gq[k, 9:30] - refs[k].get_state()[0][9:30]).max()))
            touch[k] += any((c[0], c[1]) == S.pair_geoms(a, b) for c in cons[k])
    assert (_errors(sim) == 0).all()
    sim.close()
    for k, (name, _, n, _) in enumerate(scenes):
        margin(f"{name}_max_abs_dpose", float(worst[k]), 1e-3)
        margin(f"{name}_substeps_in_contact", int(touch[k]), None, substeps=n)
    for k, (name, _, n, _) in enumerate(scenes):
        assert 2 * touch[k] >= n, (name, touch[k], n)
        assert worst[k] < 1e-3, (name, worst[k])


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS)
def test_gpu_stack_episode_matches_oracle(rows, margin):
    """The product path (PickPlaceVecEnv, expert_plan -> step) releasing red onto green: episode
    length equal to the oracle's, final red and green positions within 10 mm of it, red-green
    contact in the kernel's record along the way."""
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    n_ref, _, q_ref, green = _oracle_stack_episode()
    env = PickPlaceVecEnv(1, task=("obj_red", "bin_red"), action_mode="abs_pos", reward_type="staged", image_size=0)
    env.sim.step_rows = rows
    env.reset(seed=0)
    q, v, c, w = env.sim.get_state()
    S.put(q[0], S.GREEN, green)
    env.sim.set_state(q, v, c, w)
    env.sim.forward()
    n = touch = 0
    for _ in range(500):
        act = env.expert_plan(16)
        if int(env.fsm_state[0]) == 10:
            break
        env.step(act)
        n += 1
        touch += any((cc[0], cc[1]) == S.pair_geoms(S.RED, S.GREEN) for cc in _record(env.sim)[0][0])
    gq = env.sim.get_state()[0][0]
    assert int(env.env_error[0]) == 0
    env.close()
    d_red = float(np.linalg.norm(S.cube(gq, S.RED)[0] - S.cube(q_ref, S.RED)[0]))
    d_green = float(np.linalg.norm(S.cube(gq, S.GREEN)[0] - S.cube(q_ref, S.GREEN)[0]))
    margin("episode_length_delta", abs(n - n_ref), None, gpu=n, oracle=n_ref)
    margin("final_red_distance_m", d_red, 0.01)
    margin("final_green_distance_m", d_green, 0.01)
    margin("env_steps_in_contact", int(touch))
    assert touch > 0, "red never touched green"
    assert n == n_ref, (n, n_ref)
    assert d_red < 0.01 and d_green < 0.01, (d_red, d_green)
