"""Action-sequence rollouts with a per-step record (mmx_rollout_actions, mmx_rollout_expert_record;
PickPlaceVecEnv.rollout) against the loop they replace, byte for byte: "stepwise" below is T calls of
mmx_step (for the expert: mmx_expert_plan(16) -> mmx_step), with every sim-owned buffer copied to the host
after each call.  Slice k of every recorded array must equal the matching buffer after the k-th call, and
every buffer after the rollout the loop's final one.  No tolerances: the fused kernel runs the same
out-of-line step body per env step.

The given-action case runs 10 envs on four rollout lanes (MMX_STREAMS=4: uneven env slices, a staggered
launch plan with launches of one, two and three steps) for 11 steps with episodes of at most 4 steps, so
every env autoresets twice inside the window, mostly in the middle of a launch; the actions differ per
env and per step, so a wrong step index or env index shows."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import rollout_support as RS  # noqa: E402
from rollout_support import REL, assert_final, assert_record, digest, record_names, snapshot, to_host  # noqa: E402

N_ENVS, N_STEPS, SEED = 10, 11, 7
# (action mode, action_dim passed to the library): the relative 6D mode needs 10, passed wider
MODES = {"abs_pos": 4, REL: 12}
make_env = functools.partial(RS.make_env, n=N_ENVS, rows=128, seed=SEED)
make_actions = functools.partial(RS.make_actions, seed=1234, widths=MODES)


def stepwise(env, acts) -> list:
    """T x mmx_step; the snapshot after each."""
    snaps = []
    for k in range(acts.shape[0]):
        env.sim.step(acts[k].data_ptr(), acts.shape[2])
        snaps.append(snapshot(env))
    return snaps


# ------------------------------------------------------------------ 1. given actions
_STEPWISE: dict = {}
_FUSED: dict = {}  # (rows, lib) -> the abs_pos record of given_fused


def _given_stepwise(rows, mode):
    """The stepwise reference of the given-action case, once per (layout, mode): (snapshots, episodes at start)."""
    if (rows, mode) not in _STEPWISE:
        env = make_env(mode=mode, rows=rows)
        ep0 = snapshot(env)["episode_i"][:, 12].copy()
        acts = torch.as_tensor(make_actions(mode, N_STEPS, N_ENVS), device=env.device)
        _STEPWISE[rows, mode] = (stepwise(env, acts), ep0)
        env.close()
    return _STEPWISE[rows, mode]


def given_fused(rows, mode, lib=None):
    """The fused run of the given-action case on the build `lib` (a path; None: the product): (record, final
    buffers, launch facts)."""
    env = make_env(mode=mode, rows=rows, lib=lib)
    acts = torch.as_tensor(make_actions(mode, N_STEPS, N_ENVS), device=env.device)
    facts = {"lanes": env.sim.rollout_lanes, "launches": env.sim.rollout_launches(N_STEPS),
             "per_launch": env.sim.rollout_steps_per_launch}
    rec = to_host(env.rollout(acts, record=record_names()))
    final = snapshot(env)
    env.close()
    return rec, final, facts


@pytest.fixture(autouse=True)
def _streams4(monkeypatch):
    """Every sim of this module has four rollout lanes (MMX_STREAMS is read when a sim is created)."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    monkeypatch.setenv("MMX_STREAMS", "4")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("rows", [128, 192])
def test_given_actions_equal_stepwise(rows, mode):
    snaps, ep0 = _given_stepwise(rows, mode)
    rec, final, facts = given_fused(rows, mode)
    if mode == "abs_pos":
        _FUSED[rows, None] = rec
    # the input is worth the comparison: four staggered lanes, several launches each, multi-step launches,
    # and every env autoreset at least twice inside the window
    assert facts["lanes"] == 4
    longest = min(facts["per_launch"], (N_STEPS + 3) // 4)  # a launch's steps (the library's launch plan)
    assert 1 < longest < N_STEPS  # some launch runs several steps, and every lane needs several launches
    assert -(-N_STEPS // longest) <= facts["launches"] < N_STEPS
    assert (snaps[-1]["episode_i"][:, 12] - ep0 >= 2).all(), snaps[-1]["episode_i"][:, 12] - ep0
    assert len({s["obs"].tobytes() for s in snaps}) == N_STEPS
    assert_record(rec, snaps)
    assert_final(final, snaps[-1])


# ------------------------------------------------------------------ 2. expert record
X_ENVS, X_STEPS, X_SEED = 48, 8, 42  # tests/test_step_calls.py's setup


@pytest.mark.parametrize("rows", [128, 192])
def test_expert_record_equals_stepwise(rows):
    env = make_env(n=X_ENVS, rows=rows, seed=X_SEED, max_episode_steps=500)
    snaps, planned = [], []
    for _ in range(X_STEPS):
        a = env.expert_plan(16)
        env.sim.step(a.data_ptr(), 4)
        snaps.append(snapshot(env))
        planned.append(a.cpu().numpy())
    env.close()
    env = make_env(n=X_ENVS, rows=rows, seed=X_SEED, max_episode_steps=500)
    assert env.sim.rollout_launches(X_STEPS) < X_STEPS
    rec = to_host(env.rollout(n_steps=X_STEPS, record=record_names()))
    final = snapshot(env)
    env.close()
    assert (rec["target"] == np.stack(planned)).all()
    assert_record(rec, snaps)
    assert_final(final, snaps[-1])
    assert int(final["episode_i"][:, 10].sum()) > 0  # contacts in the record
    assert not final["episode_i"][:, 9].any()  # no error bits


# ------------------------------------------------------------------ 3. edges
@pytest.mark.parametrize("rows", [128, 192])
def test_null_record_and_reward_only(rows):
    from mujoco_manip_amd import _lib

    snaps, _ = _given_stepwise(rows, "abs_pos")
    acts = make_actions("abs_pos", N_STEPS, N_ENVS)
    env = make_env(rows=rows)
    a = torch.as_tensor(acts, device=env.device)
    env.sim.rollout_actions(a.data_ptr(), 4, N_STEPS, None)
    assert_final(snapshot(env), snaps[-1])
    env.close()
    # only the reward recorded: the other arrays exist, filled with a sentinel, and are not handed over
    env = make_env(rows=rows)
    a = torch.as_tensor(acts, device=env.device)
    arrays = {k: torch.full((N_STEPS, N_ENVS, w), -77, dtype=getattr(torch, t), device=env.device)
              for k, (w, t) in _lib.TRAJ_FIELDS.items()}
    rec = _lib.MMXTrajectory()
    rec.reward = arrays["reward"].data_ptr()
    env.sim.rollout_actions(a.data_ptr(), 4, N_STEPS, rec)
    assert_final(snapshot(env), snaps[-1])
    got = to_host(arrays)
    env.close()
    assert (got["reward"][..., 0] == np.stack([s["reward"] for s in snaps])).all()
    for k in record_names():
        if k != "reward":
            assert (got[k] == -77).all(), k


@pytest.mark.parametrize("rows", [128, 192])
def test_zero_and_one_step(rows):
    from mujoco_manip_amd import _lib

    snaps, _ = _given_stepwise(rows, "abs_pos")
    env = make_env(rows=rows)
    a = torch.as_tensor(make_actions("abs_pos", N_STEPS, N_ENVS), device=env.device)
    before = snapshot(env)
    assert env.sim.L.mmx_rollout_actions(env.sim.ptr, a.data_ptr(), 4, 0, None) == 0
    assert env.sim.L.mmx_rollout_expert_record(env.sim.ptr, 0, _lib.MMXTrajectory()) == 0
    empty = env.rollout(a[:0], record=record_names())
    assert all(v.shape[:2] == (0, N_ENVS) for v in empty.values())
    assert_final(snapshot(env), before)
    dev = env.rollout(a[:1], record=record_names())
    rec = to_host(dev)
    assert_record(rec, snaps[:1])
    assert_final(snapshot(env), snaps[0])
    # split_obs on the record gives step()'s observation keys
    from mujoco_manip_amd.vec_env import split_obs

    keys, want = split_obs(dev["obs"]), env._obs_dict()
    assert set(keys) == set(want)
    for k in want:
        assert keys[k].shape == (1, *want[k].shape) and torch.equal(keys[k][0], want[k]), k
    env.close()


@pytest.mark.parametrize("rows", [128, 192])
def test_single_env(rows):
    T = 6
    acts = make_actions("abs_pos", T, 1)
    env = make_env(n=1, rows=rows)
    snaps = stepwise(env, torch.as_tensor(acts, device=env.device))
    env.close()
    env = make_env(n=1, rows=rows)
    assert env.sim.rollout_launches(T) < T
    rec = to_host(env.rollout(torch.as_tensor(acts, device=env.device), record=record_names()))
    final = snapshot(env)
    env.close()
    assert snaps[-1]["episode_i"][0, 12] > snaps[0]["episode_i"][0, 12]  # an autoreset inside the window
    assert_record(rec, snaps)
    assert_final(final, snaps[-1])


# ------------------------------------------------------------------ 4. cameras
@pytest.mark.parametrize("expert", [False, True])
@pytest.mark.parametrize("overlap", ["1", "0"])
def test_cameras(overlap, expert, monkeypatch):
    monkeypatch.setenv("MMX_RENDER_OVERLAP", overlap)
    N, T = 3, 3
    acts = make_actions("abs_pos", T, N)
    env = make_env(n=N, image_size=32)
    assert env.sim.rollout_render_overlap == (overlap == "1")
    if expert:
        snaps = []
        for _ in range(T):
            env.sim.step(env.expert_plan(16).data_ptr(), 4)
            snaps.append(snapshot(env))
    else:
        snaps = stepwise(env, torch.as_tensor(acts, device=env.device))
    env.close()
    env = make_env(n=N, image_size=32)
    kw = {"n_steps": T} if expert else {"actions": torch.as_tensor(acts, device=env.device)}
    rec = to_host(env.rollout(record=record_names(), **kw))
    final = snapshot(env)
    env.close()
    assert final["images"].std() > 0 and final["seg"].max() > 0
    assert_record(rec, snaps)
    assert_final(final, snaps[-1])  # images and seg included: the last step's frame


# ------------------------------------------------------------------ 5. wave timing
@pytest.mark.parametrize("lib", ["libmmx_hdelay.so", "libmmx_edelay.so"])
def test_record_under_wave_delay(lib):
    """The 192-row kernel's record is written by the env wave with no barrier of its own, beside the
    helper wave: with either wave held back after barriers C and A of every substep (the test builds
    of tests/test_helper_layout.py) the record of the given-action case is the product library's."""
    from mujoco_manip_amd import _build

    if (192, None) not in _FUSED:
        _FUSED[192, None] = given_fused(192, "abs_pos")[0]
    rec, _, facts = given_fused(192, "abs_pos", _build.test_variant(lib))
    assert facts["lanes"] == 4
    assert digest(rec) == digest(_FUSED[192, None])


# ------------------------------------------------------------------ 6. refusals
def test_refusals():
    from mujoco_manip_amd import _lib

    env = make_env(n=2, mode=REL)
    before = snapshot(env)
    a = torch.zeros(3, 2, 12, device=env.device)
    L, ptr = env.sim.L, env.sim.ptr
    assert L.mmx_rollout_actions(ptr, a.data_ptr(), 9, 3, None) == -1  # the mode needs 10
    assert L.mmx_rollout_actions(ptr, None, 12, 3, None) == -1
    assert L.mmx_rollout_actions(ptr, a.data_ptr(), 12, -1, None) == -1
    assert L.mmx_rollout_expert_record(ptr, 3, _lib.MMXTrajectory()) == -1  # not an abs_pos sim
    assert L.mmx_rollout_expert_record(ptr, -1, None) == -1
    with pytest.raises(RuntimeError, match="abs_pos"):
        env.rollout(n_steps=3)
    for bad in (torch.zeros(3, 2, 9), torch.zeros(3, 3, 12), torch.zeros(2, 12), torch.zeros(3, 2, 12, 1)):
        with pytest.raises(ValueError, match="actions must be"):
            env.rollout(bad.to(env.device))
    with pytest.raises(ValueError, match="record entries"):
        env.rollout(a, record=("obs", "images"))
    with pytest.raises(ValueError):
        env.rollout()
    assert_final(snapshot(env), before)  # nothing was launched
    env.close()


# ------------------------------------------------------------------ 7. replay
def test_fused_replay_equals_loop(tmp_path):
    from mujoco_manip_amd import dataset as D
    from mujoco_manip_amd import replay as R

    keys = ["observation.state", "action.ee.pos_quat_g", "action.ee.pos_rot6d_g_rel"]
    path, _ = D.generate("user/tr", num_episodes=4, root=str(tmp_path), tasks="match", randomize_objects=True,
                         seed=5, features=keys, num_envs=4)
    for key in ("action.ee.pos_quat_g", "action.ee.pos_rot6d_g_rel"):
        loop, fused = R.replay(path, None, key), R.replay(path, None, key, fused=True)
        assert loop["episodes"] == fused["episodes"] and loop["mode"] == fused["mode"]
        for name in ("target", "ee", "err", "obs_state"):
            assert len(loop[name]) == len(fused[name]) == 4
            for x, y in zip(loop[name], fused[name]):
                assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), (key, name)
        # the simulator's own decode of each action is the report's target (fp32 against fp64 arithmetic)
        for x, y in zip(fused["sim_target"], fused["target"]):
            assert x.shape == (len(y), 4) and np.abs(x[:, :3] - y).max() < 1e-5


# ------------------------------------------------------------------ 8. one rollout driver
def _lane_launches(n, fuse, lanes):
    """Launches each lane makes for n steps (mmx_plan.h rollout_plan, as _plan_launches in tests/test_gpu.py):
    len = min(fuse, ceil(n / 4)); lane l starts with l * len / lanes steps, then launches of len, then the rest."""
    ln = max(1, min(fuse, -(-n // 4)))
    firsts = [min(n, l * ln // lanes) for l in range(lanes)]
    return [(1 if f else 0) + -(-(n - f) // ln) for f in firsts]


@pytest.mark.parametrize("case", ["lanes", "cameras_overlapped", "cameras_serial"])
def test_both_rollout_families_make_the_plans_launches(case, monkeypatch):
    """mmx_rollout_expert (the step kernel) and mmx_rollout_expert_record (the trajectory kernel) go through
    one driver: both make the step and render launches the plan defines, counted by the launch timing.
    lanes: 10 envs on four lanes, launches of at most 3 steps, 11 steps: uneven env slices, lanes 2 and 3
    start with a short launch, every lane ends with a remainder.  cameras: one lane, a step launch and a
    render launch per step; 3 steps end the overlapped path on the alternate pose buffer."""
    from mujoco_manip_amd import _lib

    if case == "lanes":
        monkeypatch.setenv("MMX_FUSE", "3")
        n, T, image_size, fuse, lanes = 10, 11, 0, 3, 4
    else:
        monkeypatch.setenv("MMX_RENDER_OVERLAP", "1" if case == "cameras_overlapped" else "0")
        n, T, image_size, fuse, lanes = 4, 3, 32, 1, 1
    per_lane = _lane_launches(T, fuse, lanes)
    if case == "lanes":
        assert per_lane == [4, 4, 5, 4]  # 3,3,3,2 / 3,3,3,2 / 1,3,3,3,1 / 2,3,3,3
    counts = []
    for record in (None, _lib.MMXTrajectory()):
        env = make_env(n=n, image_size=image_size)
        assert env.sim.rollout_lanes == lanes and env.sim.rollout_launches(T) == max(per_lane)
        if image_size:
            assert env.sim.rollout_render_overlap == (case == "cameras_overlapped")
        env.sim.kernel_timing(True)
        env.sim.rollout_expert(T, record)
        env.sim.kernel_timing(False)
        kt = env.sim.kernel_times()
        counts.append((kt["step_launches"], kt["render_launches"]))
        env.close()
    renders = T if image_size else 0  # one render launch over all envs after every step
    print(case, "step / render launches:", counts, "plan:", (sum(per_lane), renders))
    assert counts[0] == counts[1] == (sum(per_lane), renders)
