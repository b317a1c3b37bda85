"""The 192-row env-step layout (an env wave and a helper wave per env, joined by workgroup barriers)
under adversarial wave timing, with the test builds libmmx_hdelay.so / libmmx_edelay.so
(_build.TEST_VARIANTS: MMX_HELPER_DELAY holds the helper wave, or the env wave, back after barriers C and
A of every substep for longer than the other wave's longest phase; probe set 14 puts the full-prune
count and the broadphase list's displacement bound into the stats).  Whatever one wave reads from LDS
while the other still writes it differs between the two builds, and from the 128-row layout, which runs
the same phases in turn on one wave.

Each run is a sim of its own build in this process (PickPlaceVecEnv(lib=...)), one alive at a time:
  R128  libmmx_hdelay.so, 128 rows (no helper wave: the timing-free layout, carrying the probe only)
  H     libmmx_hdelay.so, 192 rows (the helper wave late)
  E     libmmx_edelay.so, 192 rows (the env wave late)
64 C3 envs, 50 lockstep expert steps; after every step a SHA-256 of (a) qpos, qvel, ctrl, (b) the last
substep's contact list, (c) the full-prune counts, (d) the displacement bounds, and the FSM states."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_ENVS, N_STEPS, SEED_ROOT = 64, 50, 42
FSM_LIFT = 4

_RUNS = {"R128": ("libmmx_hdelay.so", 128), "H": ("libmmx_hdelay.so", 192), "E": ("libmmx_edelay.so", 192)}
_DIGESTS: dict = {}


def _sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def digest_run(lib, rows):
    """N_STEPS lockstep expert steps of N_ENVS C3 envs on the build `lib`, `rows` layout -> {"steps": [[a, b, c, d, fsm]
    per step], "lift": env steps spent in the lift phase, "err": every env_error bit seen, "prunes", "substeps"}."""
    import oracle_py as O
    from mujoco_manip_amd import _lib
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(N_ENVS, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          autoreset=False, image_size=0, lib=lib)
    env.sim.step_rows = rows
    assert env.sim.step_rows == rows, env.sim.step_rows
    env.reset(seed=[O.episode_seed(SEED_ROOT, i) for i in range(N_ENVS)])
    aux0, aux1 = _lib.STAT_FIELDS.index("cyc_aux0"), _lib.STAT_FIELDS.index("cyc_aux1")
    contacts = env.sim.view("contacts", _lib.MAXCON * _lib.CON_F)
    steps, err, lift = [], 0, 0
    for t in range(N_STEPS):
        env.step(env.expert_plan(16))
        torch.cuda.synchronize()
        err |= int(np.bitwise_or.reduce(env.env_error.cpu().numpy()))
        lift += int((env.fsm_state.cpu().numpy() == FSM_LIFT).sum())
        steps.append([_sha(env.qpos, env.qvel, env.ctrl), _sha(contacts), _sha(env.stats[:, aux0]), _sha(env.stats[:, aux1]),
                      _sha(env.fsm_state)])
    out = {"steps": steps, "lift": lift, "err": err, "prunes": float(env.stats[:, aux0].sum()),
           "substeps": float(env.stats[:, 3].sum())}
    env.close()
    return out


def parity_run(lib, rows):
    """test_env_step_parity_action_modes' abs_pos case on the build `lib`: per step (actions, state, reward)."""
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    N = 4
    rng = np.random.default_rng(7)
    env = PickPlaceVecEnv(N, task=("obj_red", "bin_red"), action_mode="abs_pos", reward_type="dense", lib=lib)
    env.sim.step_rows = rows
    assert env.sim.step_rows == rows == 192, env.sim.step_rows
    env.reset(seed=0)
    out = []
    for t in range(6):
        a = np.zeros((N, env.action_dim), np.float32)
        a[:, :3] = rng.uniform(-0.05, 0.05, (N, 3)) + [0.0, 0.45, 0.42]
        a[:, -1] = float(t % 2)
        obs, rew, term, trunc, info = env.step(torch.tensor(a, device="cuda"))
        out.append((a, obs["state"].reshape(N, -1).cpu().numpy().astype(float), rew.reshape(N).cpu().numpy().astype(float)))
    env.close()
    return out


def _digests():
    """The three runs, once for the module: run -> digest_run's result."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mujoco_manip_amd import _build

    if not _DIGESTS:
        for name, (lib, rows) in _RUNS.items():
            _DIGESTS[name] = d = digest_run(_build.test_variant(lib), rows)
            assert len(d["steps"]) == N_STEPS
            print(name, "FULL_PRUNES", d["prunes"], "SUBSTEPS", d["substeps"], "LIFT_ENV_STEPS", d["lift"], "ENV_ERROR_OR", d["err"])
    return _DIGESTS


def _first_diff(x, y, k):
    """First step at which digest stream k of two runs differs, or -1."""
    return next((t for t, (p, q) in enumerate(zip(x["steps"], y["steps"])) if p[k] != q[k]), -1)


def _check_inputs(d):
    # the workload reaches the grasp's contact piles and the lift (the arm accelerating with a valid
    # list: where a stale displacement bound matters), and no run set an overflow or NaN bit
    for name, r in d.items():
        assert r["lift"] > 0, f"{name}: no env reached lift in {N_STEPS} steps"
        assert r["err"] == 0, f"{name}: env_error bits {r['err']}"


STREAMS = ("state", "contacts", "full_prunes", "disp_bound", "fsm")


def test_helper_delay_invariance():
    """Race freedom of the two-wave layout: with the helper wave held back (H) and with the env wave
    held back (E), states, contacts, full-prune counts, displacement bounds and FSM states are
    bit-identical at every one of the 50 env steps."""
    d = _digests()
    _check_inputs(d)
    first = {STREAMS[k]: _first_diff(d["H"], d["E"], k) for k in range(5)}
    print("first differing step, H vs E:", first)
    assert all(v < 0 for v in first.values()), first


def test_helper_layout_equals_single_wave_layout_under_delay():
    """Under either delay the 192-row layout computes what the 128-row layout computes on one wave
    (IK on the previous substep's position stage, the list-use decision from this substep's arm
    speeds): states, contacts, full-prune counts and displacement bounds bit-identical at every step."""
    d = _digests()
    _check_inputs(d)
    first = {f"{run}:{STREAMS[k]}": _first_diff(d[run], d["R128"], k) for run in ("H", "E") for k in range(5)}
    print("first differing step vs R128:", first)
    assert all(v < 0 for v in first.values()), first


_ORACLE_PARITY: list = []


def _oracle_parity(actions):
    """The fp64 oracle over the parity run's actions, once for the module: per step (state, reward)."""
    import oracle_py as O

    if not _ORACLE_PARITY:
        refs = [O.OracleEnv(action_mode="abs_pos", reward_type="dense", task=(0, 0)) for _ in range(4)]
        for k, r in enumerate(refs):
            r.reset(seed=k)
        for a in actions:
            res = [r.step(a[k]) for k, r in enumerate(refs)]
            _ORACLE_PARITY.append((np.stack([x[0][:11] for x in res]), np.array([x[1] for x in res])))
    return _ORACLE_PARITY


@pytest.mark.parametrize("run", ["H", "E"])
def test_helper_delay_env_step_vs_oracle(run, margin):
    """The fp64 anchor of the bit-identity tests above: test_env_step_parity_action_modes' abs_pos case
    (4 envs, 6 env steps, the same seeds and actions, the same bounds) on the delay builds' 192-row kernel.
    Measured with the race open (the kernel before barrier K, delay builds): H 3.3e-3 state / 1.08e-3
    reward (the IK on this substep's kinematics: both bounds missed), E 1.2e-6 / 9.0e-5; with barrier K
    both runs 1.2e-6 / 9.0e-5 (CHANGELOG)."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mujoco_manip_amd import _build

    lib, rows = _RUNS[run]
    steps = parity_run(_build.test_variant(lib), rows)
    ref = _oracle_parity([a for a, _, _ in steps])
    dmax, rmax = 0.0, 0.0
    for (_, got, rew), (ro, rr) in zip(steps, ref):
        dmax = max(dmax, float(np.abs(got[:, :11] - ro).max()))
        rmax = max(rmax, float(np.abs(rew - rr).max()))
        margin("max_abs_dstate", dmax, 1e-4)
        margin("max_abs_dreward", rmax, 1e-3)
        print(f"{run}: max |dstate| {dmax:.2e}, max |dreward| {rmax:.2e}")
        np.testing.assert_allclose(got[:, :11], ro, atol=1e-4)
        assert np.abs(rew - rr).max() < 1e-3
