"""DAgger rollouts inside the fused step launches (mmx_rollout_dagger; PickPlaceVecEnv.rollout_dagger,
dagger.DaggerBuffer): an MlpPolicy acts, the FSM expert plans beside it at every step, a gate picks who is obeyed.

The shapes are tests/test_traj_rollout.py's: 10 envs on four rollout lanes, 11 steps, episodes of at most 4 steps
with autoreset, so every env resets inside the window, mostly in the middle of a launch, and the lanes get uneven
env slices and launches of one, two and three steps.  The reference is the host loop the call replaces:
env.expert_plan(16) -> env.sim.step(actions[t]) on a fresh env, every sim-owned buffer copied after each step.

1. loop identity: that loop, driven with the recorded executed actions, reproduces every record slice, every
   buffer (the FSM fields of episode_i among them) and the labels, with no tolerance (both layouts, once with cameras);
2. beta = 1 is the expert: the record and the buffers of rollout(n_steps=60);
3. beta = 0 without takeover is the learner: gate 0, actions == policy_action, obs_in is what the env held, mean
   and noise as tests/test_policy_rollout.py checks them, and the labels are still the loop's: the FSM shadowed a
   learner that never obeyed it;
4. the gate's Bernoulli bit is the host restatement of u < beta (tests/dagger_ref.py) for every (t, i), fresh per
   call, repeatable, independent of the lane count;
5. the takeover bit against d2 > tau^2 in fp64 on the recorded actions;
6. either wave of the 192-row kernel held back: the same bits;
7. refusals launch nothing;
8. DaggerBuffer on the device.
"""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest

import dagger_ref
import mppi_ref
from policy_ref import U, forward64, make_spec
import rollout_support as RS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_ENVS, N_STEPS = 10, 11  # tests/test_traj_rollout.py's given-action case
make_env = functools.partial(RS.make_env, n=N_ENVS, rows=128, seed=7)
OWN = ("actions", "expert_action", "policy_action", "mean", "noise", "gate", "obs_in")
# The takeover threshold of test 5, chosen once from the distances |policy_action - expert_action| (xyz) that run 3
# (beta = 0, rows 128) recorded on an MI355X, near their median (0.2886); see test_takeover for the split it gives.
TAKEOVER_DIST = 0.29


@pytest.fixture(autouse=True)
def _streams4(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    monkeypatch.setenv("MMX_STREAMS", "4")


def policy_spec():
    """The stochastic abs_pos policy of tests/test_policy_rollout.py: seeded weights, clamped to the mode's box."""
    from mujoco_manip_amd.planner import action_box

    low, high = (np.array(v, np.float32) for v in action_box("abs_pos"))
    return make_spec(4, low=low, high=high, log_std=np.full(4, np.log(0.05), np.float32), spread=1.4, obs_gain=4.0)


_RUNS: dict = {}


def dagger_run(rows, beta, tau=0.0, steps=N_STEPS, max_episode_steps=4, image_size=0, call=0, lib=None, fresh=False):
    """rollout_dagger with everything recorded -> dict(rec, final, obs0, ep0, spec, facts); cached."""
    key = (rows, beta, tau, steps, max_episode_steps, image_size, call, lib)
    if key in _RUNS and not fresh:
        return _RUNS[key]
    from mujoco_manip_amd.policy import MlpPolicy

    spec = policy_spec()
    env = make_env(rows=rows, image_size=image_size, max_episode_steps=max_episode_steps, lib=lib)
    start = RS.snapshot(env)
    policy = MlpPolicy(**spec).bind(env)
    facts = {"lanes": env.sim.rollout_lanes, "launches": env.sim.rollout_launches(steps)}
    rec = RS.to_host(env.rollout_dagger(policy, steps, beta=beta, takeover_dist=tau, record=RS.record_names() + OWN, call=call))
    final = RS.snapshot(env)
    policy.close()
    env.close()
    run = dict(rec=rec, final=final, obs0=start["obs"], ep0=start["episode_i"][:, 12].copy(), spec=spec, facts=facts)
    if not fresh:
        _RUNS[key] = run
    return run


_LOOPS: dict = {}


def loop_run(run, rows, max_episode_steps=4, image_size=0):
    """The host loop expert_plan(16) -> step(actions[t]) on a fresh env with the run's executed actions -> (the
    snapshot after each step, the labels [T, N, 4]); cached per run."""
    if id(run) not in _LOOPS:
        env = make_env(rows=rows, image_size=image_size, max_episode_steps=max_episode_steps)
        acts = torch.as_tensor(run["rec"]["actions"], device=env.device)
        snaps, labels = [], []
        for t in range(acts.shape[0]):
            labels.append(env.expert_plan(16).cpu().numpy())
            env.sim.step(acts[t].data_ptr(), 4)
            snaps.append(RS.snapshot(env))
        env.close()
        _LOOPS[id(run)] = (run, snaps, np.stack(labels))
    return _LOOPS[id(run)][1:]


def digest(run) -> str:
    h = hashlib.sha256()
    for part in (run["rec"], run["final"]):
        for name in sorted(part):
            h.update(np.ascontiguousarray(part[name]).tobytes())
    return h.hexdigest()


def assert_loop(run, rows, **kw):
    """Record, final buffers and labels of `run` against the host loop, bit for bit."""
    from mujoco_manip_amd import _lib

    snaps, labels = loop_run(run, rows, **kw)
    rec = run["rec"]
    RS.assert_record({k: rec[k] for k in RS.record_names()}, snaps)
    RS.assert_final(run["final"], snaps[-1])  # images and seg included, with cameras
    bad = np.argwhere(rec["expert_action"] != labels)
    assert bad.size == 0, f"the label differs first at (step, env, component) = {bad[0].tolist()}"
    fsm = rec["episode_i"][:, :, _lib.EPI["fsm_state"]]
    assert len(np.unique(fsm)) >= 2  # the FSM fields compared above are not constant
    return snaps, labels


# ------------------------------------------------------------------ 1. loop identity
@pytest.mark.parametrize("rows,image_size", [(128, 0), (192, 0), (128, 16)])
def test_loop_identity(rows, image_size):
    run = dagger_run(rows, 0.5, image_size=image_size)
    rec = run["rec"]
    assert set(rec) == set(RS.record_names()) | set(OWN)
    assert rec["actions"].shape == (N_STEPS, N_ENVS, 4) and rec["gate"].shape == (N_STEPS, N_ENVS) and rec["gate"].dtype == np.int32
    assert rec["obs_in"].shape == (N_STEPS, N_ENVS, 85) and all(np.isfinite(rec[k]).all() for k in OWN if k != "gate")
    if image_size == 0:  # four staggered lanes, several launches each, some of several steps
        assert run["facts"]["lanes"] == 4 and 1 < run["facts"]["launches"] < N_STEPS
    snaps, _ = assert_loop(run, rows, image_size=image_size)
    assert (snaps[-1]["episode_i"][:, 12] - run["ep0"] >= 2).all()  # every env autoreset twice inside the window
    if image_size:
        assert run["final"]["images"].std() > 0 and run["final"]["seg"].max() > 0
    # both the learner and the expert acted, and they differ: the comparison saw a mixture
    fired = rec["gate"] != 0
    assert 0.25 <= fired.mean() <= 0.75 and (rec["policy_action"] != rec["expert_action"]).any(axis=2).all()


# ------------------------------------------------------------------ 2. beta = 1
@pytest.mark.parametrize("rows", [128, 192])
def test_beta_one_is_the_expert(rows):
    from mujoco_manip_amd import _lib

    T = 60
    run = dagger_run(rows, 1.0, steps=T, max_episode_steps=200)
    rec = run["rec"]
    env = make_env(rows=rows, max_episode_steps=200)
    want = RS.to_host(env.rollout(n_steps=T, record=RS.record_names()))
    final = RS.snapshot(env)
    env.close()
    for name in RS.record_names():
        assert rec[name].dtype == want[name].dtype and rec[name].shape == want[name].shape, name
        bad = np.argwhere(rec[name] != want[name])
        assert bad.size == 0, f"record '{name}' differs first at (step, env, ...) = {bad[0].tolist()}"
    RS.assert_final(run["final"], final)
    assert ((rec["gate"] & 1) == 1).all() and (rec["gate"] >> 1 == 0).all()
    assert (rec["actions"].view(np.uint32) == rec["expert_action"].view(np.uint32)).all()
    phases = np.bitwise_or.reduce(rec["episode_i"][:, :, _lib.EPI["fsm_phases"]].ravel())
    assert bin(int(phases)).count("1") >= 3, bin(int(phases))


# ------------------------------------------------------------------ 3. beta = 0, takeover off
@pytest.mark.parametrize("rows", [128, 192])
def test_beta_zero_is_the_learner(rows):
    run = dagger_run(rows, 0.0)
    rec, spec = run["rec"], run["spec"]
    assert (rec["gate"] == 0).all()
    assert rec["actions"].dtype == np.float32 and (rec["actions"].view(np.uint32) == rec["policy_action"].view(np.uint32)).all()
    # obs_in is what the env held before the step: the reset observation, then the record's previous slice
    assert (rec["obs_in"][0] == run["obs0"]).all() and (rec["obs_in"][1:] == rec["obs"][:-1]).all()
    mean, bound = forward64(spec, rec["obs_in"].reshape(-1, 85))
    mean, bound = mean.reshape(rec["mean"].shape), bound.reshape(rec["mean"].shape)
    frac = np.abs(rec["mean"].astype(np.float64) - mean) / np.maximum(bound, 1e-300)
    print("mean: worst fraction of the forward-error bound:", frac.max())
    assert frac.max() <= 1.0
    xi = mppi_ref.draw_array(spec["seed"], 0, N_STEPS, N_ENVS, 4)
    err = np.abs(rec["noise"].astype(np.float64) - xi).max()
    print("noise: max |device - restatement| =", err)
    assert err <= 1e-4
    std = np.exp(spec["log_std"].astype(np.float64)).astype(np.float32).astype(np.float64)
    want = np.clip(rec["mean"].astype(np.float64) + std * rec["noise"].astype(np.float64), spec["low"], spec["high"])
    assert (np.abs(rec["policy_action"].astype(np.float64) - want) / (2 * U * np.maximum(1.0, np.abs(want)))).max() <= 1.0
    # the labels are the loop's although no label was ever executed, and they are not the executed actions
    assert_loop(run, rows)
    assert (rec["expert_action"] != rec["actions"]).any(axis=2).all()
    d = np.sqrt(dagger_ref.dist2_f32(rec["policy_action"], rec["expert_action"]).astype(np.float64))
    print("xyz distance learner - expert: min / median / max =", d.min(), np.median(d), d.max())


# ------------------------------------------------------------------ 4. the gate
def test_gate_is_the_host_draw(monkeypatch):
    run = dagger_run(128, 0.5)
    rec, spec = run["rec"], run["spec"]
    u = dagger_ref.uniform_array(spec["seed"], 0, N_STEPS, N_ENVS)
    assert ((rec["gate"] & 1) == (u < 0.5)).all() and (rec["gate"] >> 1 == 0).all()
    share = (rec["gate"] & 1).mean()
    print("share of steps the expert was given:", share)
    assert 0.25 <= share <= 0.75
    want = np.where((rec["gate"] != 0)[:, :, None], rec["expert_action"], rec["policy_action"])
    assert (rec["actions"].view(np.uint32) == want.view(np.uint32)).all()
    # the same (seed, call): the same bits; call + 1: another pattern, the host's again
    again = dagger_run(128, 0.5, fresh=True)
    assert digest(again) == digest(run)
    other = dagger_run(128, 0.5, call=1)
    assert (other["rec"]["gate"] != rec["gate"]).any()
    assert ((other["rec"]["gate"] & 1) == (dagger_ref.uniform_array(spec["seed"], 1, N_STEPS, N_ENVS) < 0.5)).all()
    # one rollout lane: neither the draw nor anything else depends on lanes or the launch plan
    monkeypatch.setenv("MMX_STREAMS", "1")
    one = dagger_run(128, 0.5, fresh=True)
    assert one["facts"]["lanes"] == 1 and run["facts"]["lanes"] == 4
    assert digest(one) == digest(run)


# ------------------------------------------------------------------ 5. takeover
def test_takeover():
    """Measured on an MI355X: run 3's 110 distances span 0.078 .. 0.671 with quartiles 0.182, 0.289 (the median),
    0.395; at TAKEOVER_DIST = 0.29 the expert takes over in 61 of this run's 110 entries (55.5 %), the learner keeps
    49 (44.5 %), and no entry lies in the skipped band.  (The run's own distances differ from run 3's once the first
    takeover has changed a trajectory: here 0.078 .. 0.725, median 0.312.)"""
    tau = TAKEOVER_DIST
    run = dagger_run(128, 0.0, tau=tau)
    rec = run["rec"]
    assert ((rec["gate"] & 1) == 0).all()
    d = rec["policy_action"][:, :, :3].astype(np.float64) - rec["expert_action"][:, :, :3].astype(np.float64)
    d2 = (d * d).sum(axis=2)
    tau2 = float(np.float32(tau)) ** 2
    near = np.abs(d2 - tau2) <= 8 * 2.0 ** -24 * tau2
    take = rec["gate"] >> 1
    print("takeover share:", take.mean(), "skipped share:", near.mean())
    assert near.mean() <= 0.02
    assert (take[~near] == (d2 > tau2)[~near]).all()
    assert take.mean() >= 0.2 and (1 - take).mean() >= 0.2
    want = np.where((rec["gate"] != 0)[:, :, None], rec["expert_action"], rec["policy_action"])
    assert (rec["actions"].view(np.uint32) == want.view(np.uint32)).all()
    assert_loop(run, 128)


# ------------------------------------------------------------------ 6. wave delay
@pytest.mark.parametrize("lib", ["libmmx_hdelay.so", "libmmx_edelay.so"])
def test_under_wave_delay(lib):
    from mujoco_manip_amd import _build

    run = dagger_run(192, 0.5)
    delayed = dagger_run(192, 0.5, lib=_build.test_variant(lib))
    assert delayed["facts"]["lanes"] == 4
    assert digest(delayed) == digest(run)


# ------------------------------------------------------------------ 7. refusals
def test_refusals():
    from mujoco_manip_amd import _lib
    from mujoco_manip_amd.policy import MlpPolicy
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = make_env(n=2)
    L, sim = env.sim.L, env.sim.ptr
    policy = MlpPolicy(**policy_spec()).bind(env)
    pol = policy.device_policy.ptr
    before = RS.snapshot(env)
    arrays = {k: torch.full((3, 2, w) if w > 1 else (3, 2), -77, dtype=getattr(torch, t), device=env.device)
              for k, (w, t) in _lib.DAGGER_FIELDS.items()}
    drec = _lib.MMXDaggerRecord(**{k: v.data_ptr() for k, v in arrays.items()})
    no_actions = _lib.MMXDaggerRecord(**{k: v.data_ptr() for k, v in arrays.items() if k != "actions"})

    def cfg(beta=0.5, tau=0.0):
        return C.byref(_lib.MMXDaggerConfig(beta=beta, takeover_dist=tau))

    call = L.mmx_rollout_dagger
    assert call(None, pol, 3, 0, cfg(), C.byref(drec), None) == -1
    assert call(sim, None, 3, 0, cfg(), C.byref(drec), None) == -1
    assert call(sim, pol, 3, 0, None, C.byref(drec), None) == -1
    assert call(sim, pol, 3, 0, cfg(), None, None) == -1
    assert call(sim, pol, 3, 0, cfg(), C.byref(no_actions), None) == -1
    assert call(sim, pol, -1, 0, cfg(), C.byref(drec), None) == -1
    for beta in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
        assert call(sim, pol, 3, 0, cfg(beta=beta), C.byref(drec), None) == -1, beta
    for tau in (-1e-6, float("nan"), float("inf")):
        assert call(sim, pol, 3, 0, cfg(tau=tau), C.byref(drec), None) == -1, tau
    rel = make_env(n=2, mode=RS.REL)  # not an abs_pos sim
    rel_before = RS.snapshot(rel)
    assert call(rel.sim.ptr, pol, 3, 0, cfg(), C.byref(drec), None) == -1
    RS.assert_final(RS.snapshot(rel), rel_before)
    rel.close()
    wide = _lib.Policy(env.sim, [(np.zeros((10, 85), np.float32), None)], 0)  # an action width of 10
    assert call(sim, wide.ptr, 3, 0, cfg(), C.byref(drec), None) == -1
    wide.close()
    if torch.cuda.device_count() > 1:  # a policy created on another device
        far = PickPlaceVecEnv(2, action_mode="abs_pos", image_size=0, device=1)
        assert call(far.sim.ptr, pol, 3, 0, cfg(), C.byref(drec), None) == -1
        far.close()
    assert call(sim, pol, 0, 0, cfg(), C.byref(drec), None) == 0  # nothing to do
    RS.assert_final(RS.snapshot(env), before)  # nothing was launched
    assert all((v == -77).all() for v in arrays.values())
    # the Python layer
    for kw in ({"beta": 1.5}, {"beta": float("nan")}, {"takeover_dist": -0.1}, {"record": ("obs", "images")}):
        with pytest.raises(ValueError):
            env.rollout_dagger(policy, 3, **kw)
    with pytest.raises(ValueError, match="n_steps"):
        env.rollout_dagger(policy, -1)
    unbound = MlpPolicy(**policy_spec())
    with pytest.raises(RuntimeError, match="not bound"):
        env.rollout_dagger(unbound, 3)
    other = make_env(n=2)
    with pytest.raises(ValueError, match="bound to this env"):
        other.rollout_dagger(policy, 3)
    other.close()
    empty = env.rollout_dagger(policy, 0, record=RS.record_names() + OWN)
    assert set(empty) == set(RS.record_names()) | set(OWN) and all(v.shape[:2] == (0, 2) for v in empty.values())
    RS.assert_final(RS.snapshot(env), before)
    policy.close()
    env.close()


# ------------------------------------------------------------------ 8. the aggregate
def test_dagger_buffer():
    from mujoco_manip_amd.dagger import DEFAULT_RECORD, DaggerBuffer
    from mujoco_manip_amd.policy import MlpPolicy

    env = make_env()
    policy = MlpPolicy(**policy_spec()).bind(env)
    a = env.rollout_dagger(policy, 3, beta=0.5, call=0)
    b = env.rollout_dagger(policy, 2, beta=0.25, call=1)
    assert set(a) == set(DEFAULT_RECORD) | {"actions"}
    buf, small = DaggerBuffer(), DaggerBuffer(capacity=35)
    for rec in (a, b):
        buf.add(rec)
        small.add(rec)
    obs, lab = buf.tensors()
    assert obs.device == a["obs_in"].device and obs.shape == (50, 85) and lab.shape == (50, 4)
    assert torch.equal(obs, torch.cat([a["obs_in"].reshape(-1, 85), b["obs_in"].reshape(-1, 85)]))
    assert torch.equal(lab, torch.cat([a["expert_action"].reshape(-1, 4), b["expert_action"].reshape(-1, 4)]))
    assert torch.equal(obs[N_ENVS + 3], a["obs_in"][1, 3]) and torch.equal(lab[30 + N_ENVS + 3], b["expert_action"][1, 3])
    so, sl = small.tensors()
    assert len(small) == 35 and small.dropped == 15 and torch.equal(so, obs[15:]) and torch.equal(sl, lab[15:])
    again = DaggerBuffer(capacity=35)
    again.add(a)
    again.add(b)
    assert torch.equal(again.tensors()[0], so)  # the drop depends on the sequence of adds alone
    policy.close()
    env.close()
