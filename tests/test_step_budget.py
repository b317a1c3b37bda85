"""Time-budgeted step launches (mmx_env_step_budget_kernel, csrc/mmx_plan.h rollout_bounds): how an env's steps
fall into the launches of a rollout_expert call changes no result.

Every case rolls the same seeded envs out twice, with the switch (Sim.rollout_budget / MMX_ROLLOUT_BUDGET) on
and off, and compares every env's whole snapshot record (rng, qpos, qvel, ctrl, warm start, kinematics cache,
target, episode ints and floats, obs, reward, reward components, done) and its solver statistics bit for bit.
All cases force the 128-row layout (small batches default to the 192-row one, which always runs fixed counts)
except the one that checks the 192-row layout.  The synthetic-clock case binds its sims to the test build
libmmx_synth.so (a cost of 1 + env % 3 "ticks" per env step instead of the clock); the others run the product.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LOG = 8  # MMX_ROLLOUT_LOG: rows of the per-launch count log (24 steps at 4 per launch: 6 or 7 launches per lane)


def _env(n, max_episode_steps=500, lib=None):
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    # C3's settings (bench.py) on a few envs
    return PickPlaceVecEnv(n, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                           image_size=0, autoreset=True, max_episode_steps=max_episode_steps, lib=lib)


def _record(env):
    """Every env's snapshot record and statistics after the work queued so far, as bytes."""
    sim = env.sim
    buf = torch.zeros(sim.num_envs * sim.snapshot_bytes, dtype=torch.uint8, device="cuda")  # (records are padded to 16 bytes)
    sim.snapshot(buf.data_ptr())
    torch.cuda.synchronize()
    return buf.cpu().numpy().reshape(sim.num_envs, -1), env.stats.cpu().numpy().copy()


def _expert_run(n, steps, budget, max_episode_steps=500, rows=128, log=0, lib=None):
    """One seeded rollout_expert(steps) on the build `lib` (a path; None: the product): (records, stats, step
    counts[, per-launch counts], episode ints)."""
    import oracle_py as O
    from mujoco_manip_amd import _lib

    env = _env(n, max_episode_steps, lib)
    env.sim.step_rows = rows
    env.sim.rollout_budget = budget
    assert env.sim.rollout_budget == budget
    env.reset(seed=[O.episode_seed(42, i) for i in range(n)])
    env.rollout_expert(steps)
    rec, stats = _record(env)
    counts = env.sim.rollout_step_counts(log)
    epi = env.sim.view("episode_i", _lib.EPI_N, "<i4").cpu().numpy().copy()
    env.close()
    return rec, stats, counts, epi


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])  # the snapshot records
    # the statistics, without the phase clocks (cycle counts, which only a profile build fills)
    from mujoco_manip_amd import _lib

    keep = [k for k, name in enumerate(_lib.STAT_FIELDS) if not name.startswith("cyc_")]
    np.testing.assert_array_equal(a[1][:, keep].view(np.uint32), b[1][:, keep].view(np.uint32))
    np.testing.assert_array_equal(a[3], b[3])  # the episode ints (part of the record; named for the message)


def _uneven(log, lanes):
    """Launch rows of the log after which two envs of one lane stand at different counts."""
    n = log.shape[1]
    out = []
    for l in range(lanes):
        b0, b1 = n * l // lanes, n * (l + 1) // lanes
        out += [(l, r) for r in range(log.shape[0]) if log[r, b0:b1].min() != log[r, b0:b1].max()]
    return out


@pytest.fixture
def two_lanes(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    monkeypatch.setenv("MMX_STREAMS", "2")
    monkeypatch.setenv("MMX_FUSE", "4")
    monkeypatch.setenv("MMX_ROLLOUT_LOG", str(LOG))
    monkeypatch.delenv("MMX_ROLLOUT_BUDGET", raising=False)
    monkeypatch.delenv("MMX_PLAN", raising=False)


def test_synthetic_clock_uneven_progress_bit_identical(two_lanes, monkeypatch):
    """libmmx_synth.so, 8 envs, 2 lanes, 4 steps per launch, 24 steps: with the budget on, envs of cost 1, 2
    and 3 ticks a step leave the mid-call launches at different counts (the log shows it), every env ends at
    24, and every record equals the fixed-count run's."""
    from mujoco_manip_amd import _build

    monkeypatch.delenv("MMX_PROFILE", raising=False)
    lib = _build.test_variant("libmmx_synth.so")
    on = _expert_run(8, 24, True, log=LOG, lib=lib)
    off = _expert_run(8, 24, False, log=LOG, lib=lib)
    log = on[2][1]
    print("per-launch counts, budget on:", log.tolist())
    diff = ""
    for k, name in ((0, "record"), (1, "stats"), (3, "episode_i")):  # every byte, the phase-clock columns too
        a, b = np.ascontiguousarray(on[k]).view(np.uint8), np.ascontiguousarray(off[k]).view(np.uint8)
        if not np.array_equal(a, b):
            diff += f"{name}: envs {sorted(set(np.argwhere(a != b)[:, 0].tolist()))}; "
    assert not diff, diff
    assert on[2][0].tolist() == [24] * 8
    uneven = _uneven(log, 2)
    assert uneven, log.tolist()
    # the synthetic cost is the env's own: within a lane, a cheaper env is never behind a dearer one
    for l, r in uneven:
        b0, b1 = 8 * l // 2, 8 * (l + 1) // 2
        cost = [1 + i % 3 for i in range(b0, b1)]
        for a in range(b1 - b0):
            for b in range(b1 - b0):
                if cost[a] < cost[b]:
                    assert log[r, b0 + a] >= log[r, b0 + b], (l, r, log[r].tolist())
    # the fixed run makes no budgeted call: no counts
    assert off[2][0].tolist() == [0] * 8


def test_real_clock_bit_identical(two_lanes):
    """The product's clock, same shape: records equal, every env at 24."""
    on = _expert_run(8, 24, True, log=LOG)
    off = _expert_run(8, 24, False, log=LOG)
    print("per-launch counts, budget on:", on[2][1].tolist())
    _same(on, off)
    assert on[2][0].tolist() == [24] * 8
    assert off[2][0].tolist() == [0] * 8  # the switch off: the fixed kernel, which keeps no counts


def test_autoreset_crossings_bit_identical(two_lanes):
    """Episodes of 10 steps over a 48-step call: every env resets four times, at launch positions that differ
    between the two runs; records and episode counters equal."""
    from mujoco_manip_amd import _lib

    on = _expert_run(8, 48, True, max_episode_steps=10, log=LOG)
    off = _expert_run(8, 48, False, max_episode_steps=10, log=LOG)
    _same(on, off)
    assert on[2][0].tolist() == [48] * 8
    episodes = on[3][:, _lib.EPI["episodes"]]
    assert (episodes >= 4).all(), episodes
    np.testing.assert_array_equal(on[3][:, _lib.EPI["step_count"]], off[3][:, _lib.EPI["step_count"]])
    np.testing.assert_array_equal(episodes, off[3][:, _lib.EPI["episodes"]])


def test_switch_does_not_reach_the_other_paths(two_lanes):
    """A recorded rollout (rollout_actions with a record, 6 envs x 11 steps) and a 192-row expert rollout run
    fixed counts whatever the switch says: no budgeted call is made (the counts stay zero), and records and
    results are bit-identical with the switch on and off."""
    import oracle_py as O

    outs = []
    for budget in (True, False):
        env = _env(6)
        env.sim.step_rows = 128
        env.sim.rollout_budget = budget
        env.reset(seed=[O.episode_seed(7, i) for i in range(6)])
        g = torch.Generator(device="cpu").manual_seed(3)
        act = torch.tensor([0.0, 0.45, 0.42, 0.0]) + torch.cat([0.1 * torch.rand(11, 6, 3, generator=g) - 0.05,
                                                                torch.randint(0, 2, (11, 6, 1), generator=g).float()], 2)
        rec = env.rollout(act.cuda().contiguous(), record=("obs", "reward", "done", "episode_i", "qpos", "qvel"))
        torch.cuda.synchronize()
        outs.append(([rec[k].cpu().numpy().copy() for k in sorted(rec)], _record(env), env.sim.rollout_step_counts()))
        env.close()
    for a, b in zip(outs[0][0], outs[1][0]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    np.testing.assert_array_equal(outs[0][1][0], outs[1][1][0])
    assert outs[0][2].tolist() == [0] * 6 and outs[1][2].tolist() == [0] * 6
    on = _expert_run(8, 24, True, rows=192)
    off = _expert_run(8, 24, False, rows=192)
    _same(on, off)
    assert on[2].tolist() == [0] * 8
    # and the 192-row layout agrees with the budgeted 128-row run
    np.testing.assert_array_equal(on[0], _expert_run(8, 24, True, rows=128)[0])

