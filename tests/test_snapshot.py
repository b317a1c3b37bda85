"""Snapshot and restore of whole environments on the device (mmx_snapshot / mmx_restore;
PickPlaceVecEnv.snapshot / restore), bit for bit: a restored env must continue exactly as the env the
record was taken from did.  "Host copy" below is every sim-owned buffer copied to the host after the
queued work; comparisons are on the raw bytes, with no tolerance anywhere.

The envs run random per-env, per-step actions with episodes of at most 4 steps and autoreset, so inside
every continuation window each env is reset from its own (restored) random stream: spawns and tasks of
the new episodes only agree if the PCG64 state, its buffered half draw and the sticky episode words came
back whole."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import rollout_support as RS  # noqa: E402
from rollout_support import REL, assert_same, bits, record_names, to_host, snapshot as host  # noqa: E402

ADIM = {"abs_pos": 4, REL: 10}
SEED, OTHER_SEED = 7, 1234
make_env = functools.partial(RS.make_env, seed=SEED)


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


NOT_CAPTURED = ("contacts",)  # diagnostics of the last launch: not in a record (nor are the solver statistics)


def make_actions(mode, T, n, seed=99):
    return RS.make_actions(mode, T, n, seed=seed, widths=ADIM)


def full_rollout(env, acts):
    return to_host(env.rollout(torch.as_tensor(acts, device=env.device), record=record_names()))


# ------------------------------------------------------------------ 1. continuation
@pytest.mark.parametrize("mode", list(ADIM))
@pytest.mark.parametrize("rows", [128, 192])
def test_restored_envs_continue_as_the_original(rows, mode):
    N, PRE, WIN, EXTRA = 6, 3, 7, 2
    acts = make_actions(mode, PRE + WIN + EXTRA, N)
    env = make_env(N, mode=mode, rows=rows)
    dev = torch.as_tensor(acts, device=env.device)
    for k in range(PRE):
        env.sim.step(dev[k].data_ptr(), dev.shape[2])
    snap = env.snapshot()
    assert snap.num_envs == N and snap.rec_bytes == env.sim.snapshot_bytes and tuple(snap.data.shape) == (N, snap.rec_bytes)
    at_snap = host(env)
    rec = full_rollout(env, acts[PRE:PRE + WIN])
    final = host(env)
    # every env was reset from its own stream inside the window, and the window is not a fixed point
    assert (final["episode_i"][:, 12] > at_snap["episode_i"][:, 12]).all(), final["episode_i"][:, 12]
    assert len({rec["obs"][k].tobytes() for k in range(WIN)}) == WIN
    # disturb: two further steps, then a reset from other seeds
    for k in range(PRE + WIN, PRE + WIN + EXTRA):
        env.sim.step(dev[k].data_ptr(), dev.shape[2])
    env.reset(seed=OTHER_SEED)
    disturbed = host(env)
    assert not np.array_equal(disturbed["qpos"], at_snap["qpos"]) and not np.array_equal(disturbed["kin"], at_snap["kin"])
    obs, info = env.restore(snap)
    assert info == {} and torch.equal(obs["state"], env._obs_dict()["state"])
    assert_same(host(env), at_snap, skip=NOT_CAPTURED, what="right after the restore:")
    rec2 = full_rollout(env, acts[PRE:PRE + WIN])
    assert_same(rec2, rec, what="record of the continuation:")
    assert_same(host(env), final, what="after the continuation:")  # contacts included
    env.close()


# ------------------------------------------------------------------ 2. held cube
@pytest.mark.parametrize("rows", [128, 192])
def test_held_cube_and_fsm_states(rows):
    """The FSM expert mid-episode, envs staggered by masked resets.  On the fp64 oracle (run_episode with
    seeds 7, 8, 9) the expert closes the gripper at env steps 11-14, lifts from 21-24 and the staged
    reward's grasped flag is set at steps 24-27; so after 28 steps envs 0 and 1 hold their cube, env 3
    (reset after 10 steps: 18 into its episode) is closing the gripper and env 2 (reset after 18: 10 into
    its episode) still approaches.  The advance runs as three fused expert rollouts."""
    from mujoco_manip_amd import _lib

    N, CONT = 4, 5
    env = make_env(N, rows=rows, max_episode_steps=500)
    for steps, reset_env in ((10, 3), (8, 2), (10, None)):
        env.rollout_expert(steps)
        if reset_env is not None:
            env.synchronize()
            env.sim.reset(env_mask=[int(k == reset_env) for k in range(N)])
    snap = env.snapshot()
    at_snap = host(env)
    epi = at_snap["episode_i"]
    states, flags = epi[:, _lib.EPI["fsm_state"]], epi[:, _lib.EPI["flags"]]
    assert len(set(states.tolist())) >= 3, states
    assert (flags & 1).any(), flags  # FLAG_GRASPED: a held cube
    assert not epi[:, _lib.EPI["env_error"]].any()
    rec = to_host(env.rollout(n_steps=CONT, record=record_names()))
    final = host(env)
    env.rollout_expert(2)
    env.reset(seed=OTHER_SEED)
    env.restore(snap)
    assert_same(host(env), at_snap, skip=NOT_CAPTURED, what="right after the restore:")
    rec2 = to_host(env.rollout(n_steps=CONT, record=record_names()))
    assert_same(rec2, rec, what="record of the continuation:")
    assert_same(host(env), final, what="after the continuation:")
    env.close()


# ------------------------------------------------------------------ 3. gather
def test_gather_by_index():
    N, PRE, WIN = 6, 3, 3
    SRC = [2, 2, -1, 0, 5, 2]
    acts = make_actions("abs_pos", PRE + WIN + 1, N)
    env = make_env(N)
    dev = torch.as_tensor(acts, device=env.device)
    for k in range(PRE):
        env.sim.step(dev[k].data_ptr(), 4)
    snap = env.snapshot()
    at_snap = host(env)
    own = acts[PRE:PRE + WIN]
    ref = full_rollout(env, own)  # every env's reference continuation under its own action rows
    env.sim.step(dev[PRE + WIN].data_ptr(), 4)
    before = host(env)
    for name in ("qpos", "obs", "kin", "episode_f"):  # the kept env is worth the comparison
        assert not np.array_equal(before[name][2], at_snap[name][2]), name

    env.restore(snap, src=SRC)
    after = host(env)
    assert_same(after, before, envs=[2], what="the kept env:")  # every buffer, contacts included
    for i, r in enumerate(SRC):
        if r >= 0:
            want = {k: v[r:r + 1] for k, v in at_snap.items()}
            assert_same({k: v[i:i + 1] for k, v in after.items()}, want, skip=NOT_CAPTURED, what=f"env {i} <- record {r}:")
    # envs 0, 1 and 5 under env 2's action rows: identical, and env 2's reference continuation
    same = full_rollout(env, np.repeat(own[:, 2:3], N, axis=1))
    for i in (0, 1, 5):
        assert_same({k: v[:, i] for k, v in same.items()}, {k: v[:, 2] for k, v in ref.items()}, what=f"env {i} as env 2:")
    # under their own rows they part: the index is applied per env, not once
    env.restore(snap, src=torch.tensor(SRC, device=env.device))
    apart = full_rollout(env, own)
    assert len({apart["obs"][:, i].tobytes() for i in (0, 1, 5)}) == 3
    assert len({apart["qpos"][-1, i].tobytes() for i in (0, 1, 5)}) == 3
    # identity for one env, the others kept: env 0 from record 0 under its own rows is its own reference
    env.restore(snap, src=[0, -1, -1, -1, -1, -1])
    again = full_rollout(env, own)
    assert_same({k: v[:, 0] for k, v in again.items()}, {k: v[:, 0] for k, v in ref.items()}, what="env 0 again:")

    # indices outside the snapshot keep the env: n_records, a negative other than -1, far outside
    before = host(env)
    # (an int32 tensor reaches the kernel as it is: the range test there is the one under test)
    env.restore(snap, src=torch.tensor([N, -7, -1, 2**31 - 1, -2**31, N + 1], dtype=torch.int32, device=env.device))
    assert_same(host(env), before, what="out-of-range indices:")
    env.restore(snap, src=torch.tensor([2**32, 2**32 + 1, -1, N, -7, 2**40], device=env.device))  # int64: no wrap into range
    assert_same(host(env), before, what="out-of-range int64 indices:")
    env.close()


# ------------------------------------------------------------------ 4. one to many, across sims
def test_one_to_many_across_sims_and_layouts():
    K, PRE, T = 5, 3, 4
    pre = make_actions("abs_pos", PRE, 1, seed=5)
    cand = make_actions("abs_pos", T, K, seed=6)
    one = make_env(1)
    assert one.sim.step_rows == 192  # a 1-env sim picks the helper-wave layout
    d = torch.as_tensor(pre, device=one.device)
    for k in range(PRE):
        one.sim.step(d[k].data_ptr(), 4)
    snap = one.snapshot()
    assert snap.num_envs == 1
    many = make_env(K, rows=128, seed=OTHER_SEED)
    assert many.sim.snapshot_bytes == one.sim.snapshot_bytes
    obs, _ = many.restore(snap, src=0)
    one.synchronize()
    assert all(torch.equal(obs["state"][k], one._obs_dict()["state"][0]) for k in range(K))
    got = to_host(many.rollout(torch.as_tensor(cand, device=many.device), record=("reward", "obs")))
    assert set(got) == {"reward", "obs"}
    for k in range(K):
        one.restore(snap)
        want = to_host(one.rollout(torch.as_tensor(cand[:, k:k + 1], device=one.device), record=("reward", "obs")))
        assert_same({n: v[:, k:k + 1] for n, v in got.items()}, want, what=f"candidate {k}:")
    # the candidates were different plans from one state; the window crossed an autoreset (episodes of 4 steps)
    assert len({got["obs"][:, k].tobytes() for k in range(K)}) == K
    assert (host(many)["episode_i"][:, 12] >= 2).all()
    one.close()
    many.close()


# ------------------------------------------------------------------ 5. cameras
@pytest.mark.parametrize("effects", [(), ("shadows", "translucent_bins")])
def test_cameras_redrawn_for_the_restored_envs(effects):
    from mujoco_manip_amd import _lib

    N, T = 3, 3
    acts = make_actions("abs_pos", T + 1, N)
    env = make_env(N, image_size=32, render_effects=effects)
    dev = torch.as_tensor(acts, device=env.device)
    assert env.sim.rollout_render_overlap  # an odd rollout leaves the pose buffers swapped
    assert env.sim.snapshot_bytes == _lib.snapshot_record_bytes(True) > _lib.snapshot_record_bytes(False)
    env.rollout(dev[:T], record=())
    snap = env.snapshot()
    at_snap = host(env)
    assert at_snap["images"].std() > 0 and at_snap["seg"].max() > 0
    env.sim.step(dev[T].data_ptr(), 4)
    ref = host(env)  # the reference continuation: one further step
    env.reset(seed=OTHER_SEED)
    before = host(env)
    for i in range(N):
        assert not np.array_equal(before["images"][i], at_snap["images"][i]), i
    env.restore(snap, src=[0, -1, 2])
    after = host(env)
    assert_same(after, at_snap, skip=NOT_CAPTURED, envs=[0, 2], what="restored envs (images, seg):")
    assert_same(after, before, envs=[1], what="the kept env:")
    env.sim.step(dev[T].data_ptr(), 4)
    assert_same(host(env), ref, envs=[0, 2], what="one further step:")
    env.close()


# ------------------------------------------------------------------ 6. errors
def test_refusals_change_nothing():
    from mujoco_manip_amd import _lib
    from mujoco_manip_amd.vec_env import Snapshot

    env = make_env(3)
    a = torch.as_tensor(make_actions("abs_pos", 1, 3), device=env.device)
    env.sim.step(a[0].data_ptr(), 4)
    snap = env.snapshot()
    env.sim.step(a[0].data_ptr(), 4)
    before = host(env)
    blob = snap.data.clone()
    L, ptr, nb = env.sim.L, env.sim.ptr, env.sim.snapshot_bytes
    assert nb == L.mmx_snapshot_bytes(ptr) == _lib.snapshot_record_bytes(False) and nb % 16 == 0
    assert L.mmx_restore(ptr, blob.data_ptr(), nb + 16, 3, None) == -1  # wrong record size
    assert L.mmx_restore(ptr, blob.data_ptr(), _lib.snapshot_record_bytes(True), 3, None) == -1
    assert L.mmx_restore(ptr, None, nb, 3, None) == -1  # NULL blob
    assert L.mmx_restore(ptr, blob.data_ptr(), nb, -1, None) == -1  # negative count
    assert L.mmx_snapshot(ptr, blob.data_ptr(), nb - 16) == -1
    assert L.mmx_snapshot(ptr, None, nb) == -1
    assert L.mmx_restore(ptr, blob.data_ptr(), nb, 0, None) == 0  # no records: nothing to do
    assert_same(host(env), before, what="after the refused calls:")
    assert torch.equal(blob, snap.data)
    # facade: a camera snapshot for a camera-less env, a src of the wrong length
    cam = Snapshot(torch.zeros((3, _lib.snapshot_record_bytes(True)), dtype=torch.uint8, device=env.device))
    with pytest.raises(ValueError, match="bytes"):
        env.restore(cam)
    for bad in ([0, 1], [0, 1, 2, 0], torch.zeros((3, 1), dtype=torch.int32), [0.0, 1.0, 2.0]):
        with pytest.raises(ValueError, match="src must be"):
            env.restore(snap, src=bad)
    assert_same(host(env), before, what="after the refused facade calls:")
    # a clone is a snapshot of its own; fewer records than envs with src=None keeps the envs past them
    part = Snapshot(snap.clone().data[:2])
    env.restore(part)
    after = host(env)
    assert_same(after, before, envs=[2], what="env past the records:")
    assert not np.array_equal(after["qpos"][:2], before["qpos"][:2])
    env.close()


def test_gym_env_snapshot_restore():
    from mujoco_manip_amd.gym_env import PickPlaceGymEnv

    env = PickPlaceGymEnv(action_mode="abs_pos", reward_type="staged", image_size=0, randomize_objects=True)
    env.reset(seed=SEED)
    acts = make_actions("abs_pos", 3, 1)[:, 0]
    env.step(acts[0])
    snap = env.snapshot()
    first = env.step(acts[1])
    env.step(acts[2])
    obs, info = env.restore(snap)
    assert info == {} and obs["state"].shape == (11,)
    again = env.step(acts[1])
    assert first[1:4] == again[1:4]
    for k in first[0]:
        assert bits(first[0][k]).tobytes() == bits(again[0][k]).tobytes(), k
    env.close()
