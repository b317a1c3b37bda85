"""The contact-force pass (mmx_contact_forces) on the GPU: self-consistent, equal to the fp64 oracle's forces
within measured bounds, invisible to stepping, reproducible, and reachable through both facades.

Scenes (tests/contact_force_ref.py): the keyframe at rest; the three two-cube stacks; a held cube per colour (a
closed grasp: condim-4 torsion rows, arm-cube coupling, rows past 128, so overflow rows in HBM at the pass's
128-row record); a held cube pressed on another; one state mid move_to_bin.  Each on sims at step_rows 128 and
192 (the pass itself always uses the 128-row record; the sim's layout decides where the step kernels keep their
own overflow data, which the pass must not touch).

Bounds against the oracle.  S_MEASURED is `s` per scene class and quantity, measured on the CPU by running
tests/contact_force_ref.py as a script: the largest change of the quantity when the oracle evaluates the scene
from qpos / qvel moved by one fp32 ulp per component (16 random sign patterns), plus the change between the oracle
at 1e-13 / 200 and at the product's 1e-6 / 30.  The bound is 8 s: fp32 kinematics, collision and the row build
each add rounding of that order, while a decode error is off by the force itself.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import contact_force_ref as R  # noqa: E402
import cube_contact_scenes as S  # noqa: E402
from test_physics_kat import G, M_CUBE  # noqa: E402

pytestmark = pytest.mark.gpu
ROWS = [128, 192]
MG = M_CUBE * G
EPS32 = 2.0 ** -24
# s per scene class and quantity (force: N and N m; body_wrench: N and N m; touch: N; qacc: m/s^2 and rad/s^2), as `python tests/contact_force_ref.py` prints it
S_MEASURED = {
    "rest": {"force": 1.5034e-06, "body_wrench": 6.0135e-06, "touch": 0.0, "qacc": 2.8258e-03},
    "stack": {"force": 2.9292e-06, "body_wrench": 6.7478e-06, "touch": 0.0, "qacc": 2.8258e-03},
    "held": {"force": 1.1021e-05, "body_wrench": 2.5506e-05, "touch": 8.9882e-06, "qacc": 3.0164e-03},
    "held_on": {"force": 1.6288e-05, "body_wrench": 3.0770e-05, "touch": 1.7140e-05, "qacc": 1.2805e-02},
}
BOUND = {c: {k: 8.0 * v for k, v in q.items()} for c, q in S_MEASURED.items()}
SOLVER_TOL = 1e-6
OUTPUTS = ("contact", "force", "body_wrench", "touch", "qacc", "solve")


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


def _forces(sim):
    """One call of the pass -> {name: numpy copy of the output}."""
    sim.contact_forces()
    sim.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in sim.force_views().items()}


_RUNS = {}


def _run(rows):
    """{scene: (outputs of env, outputs of the same env at a second call)} on a sim of 8 envs at `rows`, computed
    once: the scenes go through in batches of 8, padded with the keyframe."""
    if rows not in _RUNS:
        sim = _sim(8, rows)
        scenes = R.scenes()
        out = {}
        for b0 in range(0, len(scenes), 8):
            batch = scenes[b0:b0 + 8]
            states = [s for _, _, s in batch] + [scenes[0][2]] * (8 - len(batch))
            sim.set_state(*[np.stack([np.asarray(s[k], np.float32) for s in states]) for k in range(4)])
            first, second = _forces(sim), _forces(sim)
            for e, (name, _, _) in enumerate(batch):
                out[name] = ({k: first[k][e] for k in OUTPUTS}, {k: second[k][e] for k in OUTPUTS})
        sim.close()
        _RUNS[rows] = out
    return _RUNS[rows]


def _as_result(o):
    """A device result in the reference's form (fp64), trimmed to ncon."""
    n = int(o["solve"][0])
    c = o["contact"][:n].astype(float)
    return dict(geoms=c[:, 11:13].astype(int), pos=c[:, 1:4], normal=c[:, 4:7], force=o["force"][:n].astype(float),
                body_wrench=o["body_wrench"].astype(float), touch=o["touch"].astype(float), qacc=o["qacc"].astype(float))


SCENE_NAMES = [n for n, _, _ in R.scenes()]
SCENE_CLASS = {n: c for n, c, _ in R.scenes()}


# --------------------------------------------------------------------------- 1. self-consistency, no oracle's forces
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_self_consistent(name, rows, margin):
    """The solve converged; every cube's m (qacc_lin - g) and I qacc_ang are the wrench the decode gives it, within
    what the solver's stop guarantees (gradient < tol (1 + |qfrc_smooth|), taken twice) plus the decode's rounding
    (16 x 2^-24 x the sum of the edge forces = the sum of fn); and the body wrenches are the per-contact forces
    added up with opposite signs on a contact's two bodies."""
    o = _run(rows)[name][0]
    got = _as_result(o)
    ncon, nefc, it, resid, exit_, ovf = o["solve"]
    assert exit_ == 0 and ovf == 0 and ncon == len(got["geoms"]) > 0 and nefc > 0 and resid < SOLVER_TOL, o["solve"]
    if SCENE_CLASS[name] in ("held", "held_on"):  # 4 basis rows per contact: rows past the 128 of the pass's record
        assert 4 * ncon > 128, ncon
    _, smooth = R.scene_reference(name)
    sum_f = float(got["force"][:, 0].sum())
    bound = 2 * SOLVER_TOL * (1 + smooth) + 16 * EPS32 * sum_f
    state = next(s for n, _, s in R.scenes() if n == name)
    res = R.cube_residuals(got, state[0])
    worst = max(max(r) for r in res)
    print(f"{name} rows {rows}: residual {worst:.3e} bound {bound:.3e} sum fn {sum_f:.4f} |qfrc_smooth| {smooth:.3f}")
    margin("max_cube_residual", worst, bound)
    assert worst <= bound, (res, bound)
    # the reduction: the wrenches from the per-contact output, in fp64
    e = R.oracle_at(state)
    want, scale = np.zeros((13, 6)), np.zeros(13)
    for i, (g1, g2) in enumerate(got["geoms"]):
        F, tau = got["force"][i, 1:4], got["force"][i, 4] * got["normal"][i]
        for b, sg in ((R.GEOM_BODY[g1], -1.0), (R.GEOM_BODY[g2], 1.0)):
            if b in R.BODIES:
                x = e.body(int(b))[0]
                want[R.BODIES.index(b)] += np.r_[sg * F, sg * (np.cross(got["pos"][i] - x, F) + tau)]
                scale[R.BODIES.index(b)] += np.linalg.norm(F) * (1 + np.linalg.norm(got["pos"][i] - x)) + abs(got["force"][i, 4])
    # 16 roundings of the terms' size, plus the lever's share: the body origins here are the oracle's, and fp32
    # kinematics through nine joints of a 1 m arm is off by up to 9 x 4 ulp (6e-8 m) = 2e-6 m, taken twice
    err = np.abs(got["body_wrench"] - want).max(axis=1)
    lim = (16 * EPS32 + 4e-6) * scale + 1e-12
    margin("max_wrench_sum_error_over_limit", float((err / lim).max()), 1.0)
    assert (err <= lim).all(), (err, lim)


@pytest.mark.parametrize("rows", ROWS)
def test_closed_form_loads(rows, margin):
    """A settled cube carries m g = 0.4905 N on four contacts; a two-cube stack 2 m g below and m g between."""
    run = _run(rows)
    got = _as_result(run["key"][0])
    b = BOUND["rest"]
    for o in range(3):
        sel = [i for i, g in enumerate(got["geoms"]) if tuple(g) == (S.TABLE_GEOM, S.CUBE_GEOM[o])]
        fn = got["force"][sel, 0].sum()
        margin(f"rest_load_error_{o}", abs(fn - MG), 4 * b["force"])
        assert len(sel) == 4 and abs(fn - MG) <= 4 * b["force"], (o, fn)
        w = got["body_wrench"][R.BODIES.index(16 + o)]
        assert np.abs(w - [0, 0, MG, 0, 0, 0]).max() <= b["body_wrench"], w
    b = BOUND["stack"]
    for lo, up in S.PAIRS:
        got = _as_result(run[f"stack:{lo}<{up}"][0])
        below = [i for i, g in enumerate(got["geoms"]) if tuple(g) == (S.TABLE_GEOM, S.CUBE_GEOM[lo])]
        between = [i for i, g in enumerate(got["geoms"]) if tuple(g) == S.pair_geoms(lo, up)]
        f_below, f_between = got["force"][below, 0].sum(), got["force"][between, 0].sum()
        margin(f"stack_{lo}_{up}_below_error", abs(f_below - 2 * MG), 4 * b["force"])
        margin(f"stack_{lo}_{up}_between_error", abs(f_between - MG), 8 * b["force"])
        assert (len(below), len(between)) == (4, 8)
        assert abs(f_below - 2 * MG) <= 4 * b["force"] and abs(f_between - MG) <= 8 * b["force"], (f_below, f_between)
        for o in (lo, up):
            w = got["body_wrench"][R.BODIES.index(16 + o)]
            assert np.abs(w - [0, 0, MG, 0, 0, 0]).max() <= b["body_wrench"], (o, w)


# --------------------------------------------------------------------------- 2. against the oracle
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_against_oracle(name, rows, margin):
    """body_wrench, touch and qacc directly, per-contact force after matching the contacts by geom pair and
    nearest position (every oracle contact above 1 % of the scene's largest fn must be matched), within 8 s."""
    ref, _ = R.scene_reference(name)
    got = _as_result(_run(rows)[name][0])
    d = R.differences(ref, got)
    b = BOUND[SCENE_CLASS[name]]
    for k in R.QUANTITIES:
        print(f"{name} rows {rows} {k}: {d[k]:.3e} bound {b[k]:.3e}")
        margin(k, d[k], b[k])
    bad = {k: (d[k], b[k]) for k in R.QUANTITIES if not d[k] <= b[k]}
    assert not bad, bad


# --------------------------------------------------------------------------- 3. invisible, 4. reproducible
BUFFERS = (("qpos", 30, "<f4"), ("qvel", 27, "<f4"), ("ctrl", 8, "<f4"), ("qacc_warmstart", 27, "<f4"), ("obs", 85, "<f4"),
           ("reward", 1, "<f4"), ("done", 3, "<i4"), ("reward_components", 6, "<f4"), ("episode_i", 18, "<i4"),
           ("episode_f", 28, "<f4"), ("kin", 63, "<f4"), ("stats", 19, "<f4"), ("contacts", 64 * 13, "<f4"),
           ("target", 4, "<f4"))


def _all_buffers(env):
    env.synchronize()
    out = {n: env.sim.view(n, w, t).cpu().numpy().copy().view(np.uint8) for n, w, t in BUFFERS}
    out["snapshot"] = env.snapshot().data.cpu().numpy().copy()
    return out


@pytest.mark.parametrize("rows", ROWS)
def test_pass_is_invisible_to_stepping(rows):
    """Two envs from the same seeds through 40 expert steps across the grasp, one calling contact_forces() after
    every step: every sim-owned buffer and the snapshot bytes are equal at the end; and one call leaves contacts,
    stats and qacc_warmstart as they were."""
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    envs = [PickPlaceVecEnv(4, action_mode="abs_pos", reward_type="staged", image_size=0) for _ in range(2)]
    for env in envs:
        env.sim.step_rows = rows
        env.reset(seed=11)
    grip = 0.0
    for k in range(40):
        for j, env in enumerate(envs):
            env.step(env.expert_plan())
            if j == 1:
                f = env.contact_forces()
                grip = max(grip, float(f["touch"].min(dim=1).values.max().item()))
    assert int(envs[0].fsm_state.max().item()) >= 4 and grip > 0.1, "the steps did not cross the grasp"
    before = _all_buffers(envs[1])
    envs[1].contact_forces()
    after, plain = _all_buffers(envs[1]), _all_buffers(envs[0])
    for n in before:
        assert np.array_equal(before[n], after[n]), f"a call changed {n}"
        assert np.array_equal(plain[n], after[n]), f"{n} differs from the env that never ran the pass"
    for env in envs:
        env.close()


@pytest.mark.parametrize("rows", ROWS)
def test_reproducible_and_zero_past_ncon(rows):
    for name, (a, b) in _run(rows).items():
        for k in OUTPUTS:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (name, k)
        n = int(a["solve"][0])
        assert 0 < n < 64 and not a["contact"][n:].any() and not a["force"][n:].any(), name
        assert (a["contact"][:n, 10] >= 3).all() and (a["force"][:n, 0] >= 0).all()


# --------------------------------------------------------------------------- 5. facades
def test_vec_env_facade_after_reset_step_rollout_restore():
    from mujoco_manip_amd import _lib
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    a, b = (PickPlaceVecEnv(2, action_mode="abs_pos", image_size=0) for _ in range(2))
    shapes = {"contact": (2, 64, 13), "force": (2, 64, 5), "body_wrench": (2, 13, 6), "touch": (2, 2), "qacc": (2, 27),
              "solve": (2, 6), "geoms": (2, 64, 2)}
    for env in (a, b):
        env.reset(seed=3)
    f = a.contact_forces()
    assert {k: tuple(v.shape) for k, v in f.items()} == shapes and f["geoms"].dtype == torch.int64
    n = int(f["solve"][0, 0].item())
    assert 0 <= n < 64 and (f["geoms"][0, :n] >= 0).all() and (f["geoms"][0, n:] == -1).all()
    # after a rollout the pass describes the final state: the state three step() calls reach
    a.rollout(n_steps=3)
    for _ in range(3):
        b.step(b.expert_plan())
    fa = {k: v.clone() for k, v in a.contact_forces().items()}
    fb = b.contact_forces()
    for k in shapes:
        assert torch.equal(fa[k], fb[k]), k
    # after a restore: what the pass gave at the snapshot's state
    snap = a.snapshot()
    a.step(a.expert_plan())
    assert not torch.equal(a.contact_forces()["qacc"], fa["qacc"])
    a.restore(snap)
    fr = a.contact_forces()
    for k in shapes:
        assert torch.equal(fr[k], fa[k]), k
    assert _lib.FORCE_BODIES[10] == 16
    a.close()
    b.close()


def test_gym_facade_trimmed_and_lift_phase_grip(margin):
    """PickPlaceGymEnv.contact_forces() is trimmed to ncon; during the lift phase of an expert episode both touch
    entries are positive and the held cube's vertical contact force is m (g + a_z)."""
    from mujoco_manip_amd.gym_env import PickPlaceGymEnv

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    env = PickPlaceGymEnv(task=("obj_red", "bin_red"), action_mode="abs_pos", image_size=0)
    env.reset(seed=0)
    lifts = 0
    for _ in range(80):
        env.step(env.expert_action())
        if int(env.vec_env.fsm_state[0].item()) != 4:
            continue
        f = env.contact_forces()
        n = int(f["solve"][0])
        assert f["contact"].shape == (n, 13) and f["force"].shape == (n, 5) and f["geoms"].shape == (n, 2)
        assert f["body_wrench"].shape == (13, 6) and f["touch"].shape == (2,) and f["qacc"].shape == (27,)
        assert (f["touch"] > 0).all(), f["touch"]
        want = M_CUBE * (G + float(f["qacc"][9 + 2]))
        err = abs(float(f["body_wrench"][10, 2]) - want)
        margin(f"lift_{lifts}_vertical_force_error", err, BOUND["held"]["body_wrench"])
        assert err <= BOUND["held"]["body_wrench"], (f["body_wrench"][10], want)
        lifts += 1
    assert lifts >= 3, "the episode never lifted"
    env.close()
