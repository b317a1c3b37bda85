"""Closed-loop MLP policies inside the fused step launches (mmx_policy_*, mmx_rollout_policy;
MlpPolicy, PickPlaceVecEnv.rollout_policy).

The shapes are tests/test_traj_rollout.py's: 10 envs on four rollout lanes, 11 steps, episodes of at most 4
steps with autoreset, so every env resets twice inside the window, mostly in the middle of a launch, and the
lanes get uneven env slices and launches of one, two and three steps.

1. replay identity: rollout(actions=rec["actions"]) from the same start gives every recorded array and every
   sim-owned buffer bit for bit (both layouts, two action modes, once with cameras);
2. the actions are the policy of the observations the envs had: the recorded mean against an fp64 evaluation of
   the network on the reset observation (t = 0) or rec["obs"][t - 1] (after an autoreset: the new episode's
   first observation), within the forward-error bound below; actions == clip(mean) exactly;
3. the network alone (mmx_policy_eval) at the widths and depths where the loops change, against fp64;
4. the tanh form on a grid of arguments, against ACT_EPS;
5. the noise: the draw of tests/mppi_ref.py, repeatable, fresh per call, independent of the lane count;
6. either wave of the 192-row kernel held back: the same bits;
7. refusals launch nothing.

Forward-error bound (computed per case, never fixed): with u = 2^-24, a layer of n inputs adds
2 (n + 2) u (|W| |x| + |b|) (the fused accumulation's n + 1 roundings; the factor 2 covers fused against unfused
products and the two roundings of the normalised input) to |W| times the incoming error; a tanh unit adds
ACT_EPS = 8 u (v_exp_f32 and v_rcp_f32 within one ulp each, and the rounding of the exponent's argument, which
the form damps by |x| e^2x / (1 + e^2x)^2 < 0.5); both activations are 1-Lipschitz.
Measured on an MI355X (profiles/r16_policy_margins.json): mmx_policy_eval at most 1.5 % of the bound, the rollout's
mean 0.004 %, tanh 0.31 ACT_EPS, the noise 2.7e-7 from the restatement (bound 1e-4), a noisy action 0.25 of its bound.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import mppi_ref
from policy_ref import ACT_EPS, U, forward64, make_spec
import rollout_support as RS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_ENVS, N_STEPS, SEED, REL = 10, 11, 7, RS.REL  # tests/test_traj_rollout.py's given-action case
make_env = functools.partial(RS.make_env, n=N_ENVS, rows=128, seed=SEED)
MARGINS: dict = {}  # name -> the worst fraction of its bound seen in this session


def note(name, value):
    MARGINS[name] = max(MARGINS.get(name, 0.0), float(value))
    print(f"{name}: {value:.4g}")
    path = os.environ.get("MMX_POLICY_MARGINS")
    if path:
        with open(path, "w") as f:
            json.dump(MARGINS, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _streams4(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    monkeypatch.setenv("MMX_STREAMS", "4")


# ------------------------------------------------------------------ policies and the fp64 reference
def mode_box(mode):
    """(low, high) the test's policies clamp to: the mode's own box for abs_pos; for the relative 6D mode a small
    box around "stay here, identity rotation" (the trajectory test's action range), so no env is thrown about."""
    if mode == "abs_pos":
        from mujoco_manip_amd.planner import action_box

        low, high = action_box(mode)
        return np.array(low, np.float32), np.array(high, np.float32)
    ident = np.array([1, 0, 0, 0, 1, 0], np.float32)
    low = np.concatenate([np.full(3, -0.1), ident - 0.05, [0.0]]).astype(np.float32)
    high = np.concatenate([np.full(3, 0.1), ident + 0.05, [1.0]]).astype(np.float32)
    return low, high


def make_policy(spec):
    from mujoco_manip_amd.policy import MlpPolicy

    return MlpPolicy(**spec)


# ------------------------------------------------------------------ the closed-loop run, once per configuration
_RUNS: dict = {}


def policy_run(rows, mode, stochastic=False, image_size=0, call=0, lib=None):
    """rollout_policy with everything recorded, on the build `lib` of the library (a path; None: the product)
    -> dict(rec, final, obs0, spec, facts); cached."""
    key = (rows, mode, stochastic, image_size, call, lib)
    if key in _RUNS:
        return _RUNS[key]
    A = 4 if mode == "abs_pos" else 10
    low, high = mode_box(mode)
    # (spread and gain chosen on the envs' own observations: 15 % and 11 % of the outputs leave the two boxes)
    spec = make_spec(A, low=low, high=high, log_std=np.full(A, np.log(0.05), np.float32) if stochastic else None,
                     spread=1.4, obs_gain=4.0)
    env = make_env(mode=mode, rows=rows, image_size=image_size, lib=lib)
    obs0 = env._obs.cpu().numpy().copy()
    policy = make_policy(spec).bind(env)
    facts = {"lanes": env.sim.rollout_lanes, "launches": env.sim.rollout_launches(N_STEPS),
             "per_launch": env.sim.rollout_steps_per_launch}
    rec = RS.to_host(env.rollout_policy(policy, N_STEPS, record=RS.record_names() + ("mean", "noise"), call=call))
    final = RS.snapshot(env)
    policy.close()
    env.close()
    _RUNS[key] = dict(rec=rec, final=final, obs0=obs0, spec=spec, facts=facts)
    return _RUNS[key]


def digest(run) -> str:
    h = hashlib.sha256()
    for name in sorted(run["rec"]):
        h.update(np.ascontiguousarray(run["rec"][name]).tobytes())
    for name in sorted(run["final"]):
        h.update(np.ascontiguousarray(run["final"][name]).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------ 1. replay identity
@pytest.mark.parametrize("rows,mode,image_size", [(128, "abs_pos", 0), (192, "abs_pos", 0), (128, REL, 0), (192, REL, 0),
                                                  (128, "abs_pos", 16)])
def test_replay_identity(rows, mode, image_size):
    run = policy_run(rows, mode, image_size=image_size)
    rec, spec = run["rec"], run["spec"]
    assert rec["actions"].shape == (N_STEPS, N_ENVS, len(spec["low"])) and np.isfinite(rec["actions"]).all()
    if image_size == 0:  # four staggered lanes, several launches each, some of several steps
        assert run["facts"]["lanes"] == 4 and 1 < run["facts"]["launches"] < N_STEPS
    env = make_env(mode=mode, rows=rows, image_size=image_size)
    ep0 = RS.snapshot(env)["episode_i"][:, 12].copy()
    replay = RS.to_host(env.rollout(torch.as_tensor(rec["actions"], device=env.device), record=RS.record_names()))
    final = RS.snapshot(env)
    env.close()
    assert (final["episode_i"][:, 12] - ep0 >= 2).all()  # every env autoreset twice inside the window
    for name in RS.record_names():
        assert rec[name].dtype == replay[name].dtype and rec[name].shape == replay[name].shape, name
        bad = np.argwhere(rec[name] != replay[name])
        assert bad.size == 0, f"record '{name}' differs first at (step, env, ...) = {bad[0].tolist()}"
    if image_size:
        assert final["images"].std() > 0 and final["seg"].max() > 0
    RS.assert_final(run["final"], final)  # images and seg included, with cameras
    # the clamp was seen to act, and most outputs needed none
    outside = (rec["mean"] < spec["low"]) | (rec["mean"] > spec["high"])
    print("network outputs outside the box:", outside.mean())
    assert 0 < outside.mean() < 0.5


# ------------------------------------------------------------------ 2. the policy of the observations the env had
def _launch_starts(T, fuse, lanes):
    """Per lane, the rollout steps at which its launches start (mmx_plan.h rollout_plan, as _lane_launches of
    tests/test_traj_rollout.py)."""
    ln = max(1, min(fuse, -(-T // 4)))
    out = []
    for l in range(lanes):
        first = min(T, l * ln // lanes)
        out.append(sorted({0} | set(range(first, T, ln))))
    return out


@pytest.mark.parametrize("rows", [128, 192])
def test_actions_are_the_policy_of_the_observations(rows):
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    run = policy_run(rows, "abs_pos")
    rec, spec = run["rec"], run["spec"]
    inputs = np.concatenate([run["obs0"][None], rec["obs"][:-1]])  # [T, N, 85]: what env n held before step t
    mean, bound = forward64(spec, inputs.reshape(-1, 85))
    mean, bound = mean.reshape(rec["mean"].shape), bound.reshape(rec["mean"].shape)
    frac = np.abs(rec["mean"].astype(np.float64) - mean) / np.maximum(bound, 1e-300)
    note(f"rollout_mean_rows{rows}", frac.max())
    assert frac.max() <= 1.0
    want = np.clip(rec["mean"], spec["low"], spec["high"])  # float32, on the device's own mean
    assert want.dtype == np.float32 and (rec["actions"] == want).all()
    assert (rec["noise"] == 0).all()
    # the premise: an env autoreset at step t, step t + 1 is inside a launch (not its first step), and the ended
    # episode's final observation (an env without autoreset, stepped with the same actions) would have given a
    # mean that differs from the recorded one by more than the bound
    starts = _launch_starts(N_STEPS, run["facts"]["per_launch"], 4)
    lane_of = [next(l for l in range(4) if N_ENVS * l // 4 <= n < N_ENVS * (l + 1) // 4) for n in range(N_ENVS)]
    ended = (rec["done"][:, :, 0] | rec["done"][:, :, 1]) != 0
    interior = [(t, n) for t in range(N_STEPS - 1) for n in range(N_ENVS) if ended[t, n] and t + 1 not in starts[lane_of[n]]]
    assert interior, "no autoreset ahead of an interior step of a launch"
    t0 = min(t for t, _ in interior)
    env = PickPlaceVecEnv(N_ENVS, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          max_episode_steps=4, autoreset=False, image_size=0)
    env.sim.step_rows = rows
    env.reset(seed=SEED)
    kept = RS.to_host(env.rollout(torch.as_tensor(rec["actions"][:t0 + 1], device=env.device), record=("obs", "done")))
    env.close()
    seen = 0
    for t, n in interior:
        if t != t0 or ended[:t, n].any():
            continue
        assert kept["done"][t, n, 0] or kept["done"][t, n, 1]
        stale, _ = forward64(spec, kept["obs"][t, n][None])
        gap = np.abs(stale[0] - rec["mean"][t + 1, n].astype(np.float64))
        seen += int((gap > bound[t + 1, n]).any())
    assert seen > 0, "the reset observation does not move the policy's output past the bound"


# ------------------------------------------------------------------ 3. the network alone
_SIM = {}


def eval_sim():
    if "env" not in _SIM:
        _SIM["env"] = make_env(n=1)
    return _SIM["env"]


WIDTHS = (1, 63, 64, 65, 255, 256)


@pytest.mark.parametrize("A", [4, 10])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_network_arithmetic(activation, A):
    env = eval_sim()
    rng = np.random.default_rng(5)
    obs = rng.uniform(-2.0, 2.0, (7, 85)).astype(np.float32)
    obs[:, 17] = np.float32(3e30)  # dropped by a zero scale: it must not reach the output
    worst = 0.0
    for depth in (1, 2, 3, 4):
        for w in WIDTHS if depth > 1 else (None,):
            for bias in (True, False):
                hidden = () if depth == 1 else (w,) + (WIDTHS[(WIDTHS.index(w) + 2) % 6],) * (depth - 2)
                spec = make_spec(A, hidden=hidden, activation=activation, bias=bias, seed=depth * 1000 + (w or 0))
                spec["obs_scale"][17] = 0.0
                policy = _bind_any(make_policy(dict(spec, low=None, high=None)), env)
                got = policy.eval(torch.as_tensor(obs, device=env.device)).cpu().numpy()
                policy.close()
                want, bound = forward64(spec, obs)
                assert got.shape == (7, A) and np.isfinite(got).all(), (depth, w, bias)
                frac = (np.abs(got.astype(np.float64) - want) / np.maximum(bound, 1e-300)).max()
                assert frac <= 1.0, (depth, w, bias, frac)
                assert np.abs(want).max() < 1e3  # 3e30 reached nothing
                worst = max(worst, frac)
    note(f"eval_{activation}_A{A}", worst)


def _bind_any(policy, env):
    """The device object for mmx_policy_eval alone, whatever the env's action dimension (bind() insists on a
    match because it prepares a rollout)."""
    from mujoco_manip_amd import _lib

    policy._dev = _lib.Policy(env.sim, policy.layers, _lib.POLICY_ACTIVATIONS.index(policy.activation), policy.obs_shift,
                              policy.obs_scale, None, None, None, 0)
    policy._env = env
    return policy


# ------------------------------------------------------------------ 4. tanh
def test_tanh_sweep():
    env = eval_sim()
    grid = [0.0] + [s * 2.0 ** e for e in range(-20, 5) for s in (1, -1)] + [s * v for v in (20.0, 88.0, 100.0) for s in (1, -1)]
    grid = np.array(grid + np.linspace(-10.0, 10.0, 256 - len(grid)).tolist(), np.float32)  # the rest: a plain sweep
    assert len(grid) == 256 and 16.0 in grid and np.float32(2.0 ** -20) in grid
    hidden = (np.zeros((256, 85), np.float32), grid)  # W1 = 0: hidden unit j is tanh(grid[j]) exactly
    got = np.zeros(256, np.float32)
    for j0 in range(0, 256, 10):  # one-hot output rows select ten hidden units at a time
        js = np.arange(j0, min(j0 + 10, 256))
        sel = np.zeros((len(js), 256), np.float32)
        sel[np.arange(len(js)), js] = 1
        policy = _bind_any(make_policy(dict(layers=[hidden, (sel, None)], activation="tanh")), env)
        got[js] = policy.eval(torch.ones(1, 85, device=env.device)).cpu().numpy()[0]
        policy.close()
    assert np.isfinite(got).all() and ((got.view(np.uint32) & 0x7F800000) != 0x7F800000).all()
    err = np.abs(got.astype(np.float64) - np.tanh(grid.astype(np.float64)))
    note("tanh_abs_error_over_ACT_EPS", err.max() / ACT_EPS)
    assert err.max() <= ACT_EPS
    assert (got[grid == 100.0] == 1.0).all() and (got[grid == -100.0] == -1.0).all() and (got[grid == 88.0] == 1.0).all()
    assert (got[grid == 0.0] == 0.0).all()


# ------------------------------------------------------------------ 5. noise
def test_noise(monkeypatch):
    run = policy_run(128, "abs_pos", stochastic=True)
    rec, spec = run["rec"], run["spec"]
    A = 4
    xi = mppi_ref.draw_array(spec["seed"], 0, N_STEPS, N_ENVS, A)
    err = np.abs(rec["noise"].astype(np.float64) - xi).max()
    note("noise_abs_error", err)
    assert err <= 1e-4
    std = np.exp(spec["log_std"].astype(np.float64)).astype(np.float32).astype(np.float64)
    want = np.clip(rec["mean"].astype(np.float64) + std * rec["noise"].astype(np.float64), spec["low"], spec["high"])
    frac = np.abs(rec["actions"].astype(np.float64) - want) / (2 * U * np.maximum(1.0, np.abs(want)))
    note("noisy_action_fraction", frac.max())
    assert frac.max() <= 1.0
    # the same (seed, call): the same bits; call + 1: every element differs
    key = (128, "abs_pos", True, 0, 0, None)
    _RUNS.pop(key)
    again = policy_run(128, "abs_pos", stochastic=True)
    assert digest(again) == digest(run)
    other = policy_run(128, "abs_pos", stochastic=True, call=1)
    assert (other["rec"]["noise"] != rec["noise"]).all()
    # one rollout lane: the draw does not depend on lanes or the launch plan
    monkeypatch.setenv("MMX_STREAMS", "1")
    _RUNS.pop(key)
    one = policy_run(128, "abs_pos", stochastic=True)
    _RUNS[key] = run  # (the cached run stays the four-lane one)
    assert one["facts"]["lanes"] == 1 and run["facts"]["lanes"] == 4
    assert digest(one) == digest(run)


# ------------------------------------------------------------------ 6. wave delay
@pytest.mark.parametrize("lib", ["libmmx_hdelay.so", "libmmx_edelay.so"])
def test_under_wave_delay(lib):
    from mujoco_manip_amd import _build

    run = policy_run(192, "abs_pos")
    delayed = policy_run(192, "abs_pos", lib=_build.test_variant(lib))
    assert delayed["facts"]["lanes"] == 4
    assert digest(delayed) == digest(run)


# ------------------------------------------------------------------ 7. arguments
def test_refusals():
    import ctypes as C

    from mujoco_manip_amd import _lib
    from mujoco_manip_amd.policy import MlpPolicy
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = make_env(n=2)
    L, sim = env.sim.L, env.sim.ptr
    before = RS.snapshot(env)
    W = [np.zeros((8, 85), np.float32), np.zeros((4, 8), np.float32)]

    def cfg(n_layers=2, widths=(8, 4), activation=0, weights=W):
        c = _lib.MMXPolicyConfig(n_layers=n_layers, activation=activation)
        for k, w in enumerate(widths):
            c.width[k] = w
        for k, w in enumerate(weights):
            c.weight[k] = None if w is None else w.ctypes.data
        return c

    out = C.c_void_p()
    good = cfg()
    for bad in (cfg(n_layers=0), cfg(n_layers=5), cfg(widths=(0, 4)), cfg(widths=(257, 4)), cfg(widths=(8, 11)),
                cfg(weights=(W[0], None)), cfg(activation=2)):
        assert L.mmx_policy_create(sim, C.byref(bad), C.byref(out)) == -1 and not out.value
    assert L.mmx_policy_create(None, C.byref(good), C.byref(out)) == -1 and not out.value
    assert L.mmx_policy_create(sim, None, C.byref(out)) == -1 and not out.value
    assert L.mmx_policy_create(sim, C.byref(good), None) == -1
    assert L.mmx_policy_create(sim, C.byref(good), C.byref(out)) == 0 and out.value
    acts = torch.full((3, 2, 4), -77.0, device=env.device)
    prec = _lib.MMXPolicyRecord(actions=acts.data_ptr())
    obs = torch.zeros(2, 85, device=env.device)
    mean = torch.full((2, 4), -77.0, device=env.device)
    assert L.mmx_policy_eval(None, obs.data_ptr(), 2, mean.data_ptr()) == -1
    assert L.mmx_policy_eval(out, None, 2, mean.data_ptr()) == -1
    assert L.mmx_policy_eval(out, obs.data_ptr(), 2, None) == -1
    assert L.mmx_policy_eval(out, obs.data_ptr(), -1, mean.data_ptr()) == -1
    assert L.mmx_policy_eval(out, obs.data_ptr(), 0, mean.data_ptr()) == 0
    assert L.mmx_rollout_policy(None, out, 3, 0, C.byref(prec), None) == -1
    assert L.mmx_rollout_policy(sim, None, 3, 0, C.byref(prec), None) == -1
    assert L.mmx_rollout_policy(sim, out, 3, 0, None, None) == -1
    assert L.mmx_rollout_policy(sim, out, 3, 0, C.byref(_lib.MMXPolicyRecord()), None) == -1
    assert L.mmx_rollout_policy(sim, out, -1, 0, C.byref(prec), None) == -1
    assert L.mmx_rollout_policy(sim, out, 0, 0, C.byref(prec), None) == 0
    rel = make_env(n=2, mode=REL)  # the policy has 4 outputs, this sim's actions 10
    assert L.mmx_rollout_policy(rel.sim.ptr, out, 3, 0, C.byref(prec), None) == -1
    RS.snapshot(rel)
    rel.close()
    if torch.cuda.device_count() > 1:  # a policy created on another device
        far = PickPlaceVecEnv(2, action_mode="abs_pos", image_size=0, device=1)
        assert L.mmx_rollout_policy(far.sim.ptr, out, 3, 0, C.byref(prec), None) == -1
        far.close()
    RS.assert_final(RS.snapshot(env), before)  # nothing was launched
    assert (acts == -77).all() and (mean == -77).all()
    L.mmx_policy_destroy(out)
    L.mmx_policy_destroy(None)
    # the Python layer
    policy = MlpPolicy([(W[0], None), (W[1], None)])
    with pytest.raises(RuntimeError, match="not bound"):
        env.rollout_policy(policy, 3)
    policy.bind(env)
    with pytest.raises(ValueError, match="record entries"):
        env.rollout_policy(policy, 3, record=("obs", "images"))
    with pytest.raises(ValueError, match="n_steps"):
        env.rollout_policy(policy, -1)
    with pytest.raises(ValueError, match="obs must be"):
        policy.eval(torch.zeros(2, 84))
    other = make_env(n=2)
    with pytest.raises(ValueError, match="bound to this env"):
        other.rollout_policy(policy, 3)
    other.close()
    wide = MlpPolicy([(np.zeros((10, 85), np.float32), None)])
    with pytest.raises(ValueError, match="action_dim"):
        wide.bind(env)
    RS.assert_final(RS.snapshot(env), before)
    empty = env.rollout_policy(policy, 0, record=RS.record_names() + ("mean", "noise"))
    assert set(empty) == set(RS.record_names()) | {"actions", "mean", "noise"}
    assert all(v.shape[:2] == (0, 2) for v in empty.values())
    RS.assert_final(RS.snapshot(env), before)
    policy.close()
    env.close()
