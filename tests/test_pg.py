"""Policy-gradient fits on the device (mmx_gae, mmx_policy_fit_pg, mmx_policy_set_log_std; PickPlaceVecEnv.gae,
MlpPolicy.fit_pg / set_log_std, MlpCritic).

The gate is tests/test_policy_fit.py's: err(T) = max |T - T64| / max |T64| against the fp64 restatement
(tests/pg_ref.py), err_gpu <= 8 max(err_yardstick, 2^-24) per tensor.  Every test prints its worst fraction of the
gate; MMX_FIT_MARGINS=<path> collects them.  PPO's clip test is discontinuous, so every case that is compared with
the reference first asserts, on the fp64 reference alone and before the device is touched, that no sample's ratio
lies within 1e-4 (relative) of 1 - clip or 1 + clip and that no advantage is 0 (pg_ref.assert_clip_condition): a
condition on the inputs.  No sample is left out of a comparison.

1. GAE: shapes around the 64-lane wave and the 256-thread workgroup, every done pattern, the exact cut, normalisation;
2. gradients: one SGD step at lr = 1, shuffle = 0, so the exported weight change is the gradient, over nets, action
   widths and batches around the sample tile (16), the staging block (32) and the K chunk (512), and B > n;
3. the three statistics and ten shuffled Adam steps;
4. reproducibility, bit for bit, and the optimiser state shared with the MSE fit;
5. in place and ordered: eval and a rollout queued right behind fit_pg run the new weights; set_log_std;
6. a critic fitted on GAE's returns;
7. every MMX_EINVAL case, with the policy untouched;
8. direction: rewarding positive noise in component 0 raises that component's mean."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import pg_ref as R
import policy_fit_ref as FR
from policy_ref import make_spec
import rollout_support as RS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
CLIP = 0.2
make_env = functools.partial(RS.make_env, n=10, rows=128, seed=7)
MARGINS: dict = {}


def note(name, value):
    MARGINS[name] = max(MARGINS.get(name, 0.0), float(value))
    print(f"{name}: {value:.4g}")
    path = os.environ.get("MMX_FIT_MARGINS")
    if path:
        with open(path, "w") as f:
            json.dump(MARGINS, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _streams4(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    monkeypatch.setenv("MMX_STREAMS", "4")


@pytest.fixture(scope="module")
def envs():
    """The sims the sim-less tests run on, by action dimension (abs_pos has 4, the relative 6D mode 10)."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    made = {4: make_env(), 10: make_env(mode=RS.REL)}
    yield made
    for e in made.values():
        e.close()


@pytest.fixture
def env(envs):
    return envs[4]


def bind(spec, env):
    from mujoco_manip_amd.policy import MlpPolicy

    return MlpPolicy(**spec).bind(env)


def dev(a, env, dtype=F32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype), device=env.device)


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def gate(name, got, want64, yard):
    """Asserts err(got) <= 8 max(err(yard), 2^-24); returns the fraction of the gate."""
    e, y = R.err(got, want64), R.err(yard, want64)
    frac = e / (8 * max(y, R.U))
    assert frac <= 1.0, f"{name}: err {e:.3e}, yardstick {y:.3e}, {frac:.2f} of the gate"
    return frac


def spec_layers(spec):
    return [(W, np.zeros(W.shape[0], F32) if b is None else b) for W, b in spec["layers"]]


def words(layers):
    return np.concatenate([np.concatenate([W.ravel(), b.ravel()]) for W, b in layers]).view(np.uint32)


def dev_case(case, env):
    obs, mean_old, noise, adv, _ = case
    return [dev(a, env) for a in (obs, mean_old, noise, adv)]


# ------------------------------------------------------------------ 1. GAE
@pytest.mark.parametrize("T,N", R.GAE_SHAPES)
def test_gae(env, T, N):
    reward, done, value, value_last = R.make_gae_case(T, N)
    (a64, r64), (a32, r32) = (R.gae(reward, done, value, value_last, 0.99, 0.95, f) for f in (False, True))
    args = [dev(reward, env), dev(done, env, np.int32), dev(value, env), dev(value_last, env)]
    adv, ret = env.gae(*args, gamma=0.99, lam=0.95)
    adv2, ret2 = env.gae(*args, gamma=0.99, lam=0.95)
    assert adv.shape == (T, N) and (bits(adv) == bits(adv2)).all() and (bits(ret) == bits(ret2)).all()
    adv, ret = adv.cpu().numpy(), ret.cpu().numpy()
    worst = max(gate("adv", adv, a64, a32), gate("ret", ret, r64, r32))
    # the cut is exact: whatever follows an env's ended step does not reach that step or any before it
    end = (done[..., 0] != 0) | (done[..., 1] != 0)
    assert end[0, 0] and (N == 1 or end[T - 1, 1])
    after = np.cumsum(end, 0) - end > 0  # strictly behind the env's first ended step
    reward2, value2 = np.where(after, reward + 5, reward).astype(F32), np.where(after, -2 * value - 1, value).astype(F32)
    last2 = np.where(end.any(0), value_last + 9, value_last).astype(F32)
    adv3, ret3 = env.gae(dev(reward2, env), args[1], dev(value2, env), dev(last2, env), gamma=0.99, lam=0.95)
    keep = ~after & end.any(0)[None, :]
    assert keep.any() and (adv3.cpu().numpy()[keep].view(np.uint32) == adv[keep].view(np.uint32)).all()
    assert (ret3.cpu().numpy()[keep].view(np.uint32) == ret[keep].view(np.uint32)).all()
    if after.any():
        assert (adv3.cpu().numpy()[after] != adv[after]).any()
    # normalised: against the reference, mean 0 and variance 1, the returns untouched, the same bits again
    nadv, nret = env.gae(*args, gamma=0.99, lam=0.95, normalize=True)
    nadv2, _ = env.gae(*args, gamma=0.99, lam=0.95, normalize=True)
    assert (bits(nadv) == bits(nadv2)).all() and (bits(nret) == ret.view(np.uint32)).all()
    nadv = nadv.cpu().numpy()
    n64, n32 = R.normalise(a64, False), R.normalise(a32, True)
    worst = max(worst, gate("normalised adv", nadv, n64, n32))
    if T * N > 1:
        g, y = nadv.astype(np.float64), n32.astype(np.float64)
        m_frac = abs(g.mean()) / (8 * max(abs(y.mean()), R.U))
        v_frac = abs(g.var() - 1) / (8 * max(abs(y.var() - 1), R.U))
        assert m_frac <= 1 and v_frac <= 1, (g.mean(), g.var(), y.mean(), y.var())
        worst = max(worst, m_frac, v_frac)
    else:
        assert (nadv == 0).all()  # one entry: x - mean = 0
    note(f"gae T={T} N={N}", worst)


# ------------------------------------------------------------------ 2. gradients
def pg_step_case(env, spec, case, B, name):
    """One SGD step at lr = 1 on the first B samples in order (wrapping when B > n): the exported weight change
    against the fp64 gradient, and the loss."""
    obs, mean_old, noise, adv, std = case
    idx = R.batch_indices(0, 0, 0, B, len(obs))
    n64, n32 = R.PgNet(spec, False), R.PgNet(spec, True)
    R.assert_clip_condition(n64, case, idx, CLIP)  # before the device is touched
    pack = (mean_old[idx], noise[idx], adv[idx], std, CLIP)
    s64, s32 = n64.step(obs[idx], pack, "sgd", lr=1.0), n32.step(obs[idx], pack, "sgd", lr=1.0)
    p = bind(spec, env)
    stats = p.fit_pg(*dev_case(case, env), 1, clip=CLIP, batch=B, lr=1.0, optimizer="sgd", shuffle=False)
    after = p.weights()
    stats = stats.cpu().numpy()
    p.close()
    assert stats.shape == (1, 3)
    worst = gate(f"{name} loss", stats[:, 0], s64[:1], s32[:1])
    assert abs(stats[0, 2] - s64[2]) < 0.5 / B, "a sample fell on the other side of the clip"
    for l, ((W0, b0), (W, b), (W64, b64), (W32, b32)) in enumerate(zip(spec_layers(spec), after, n64.layers, n32.layers)):
        for kind, w0, w, w64, w32 in (("W", W0, W, W64, W32), ("b", b0, b, b64, b32)):
            w0 = w0.astype(np.float64)
            if not np.any(w64 - w0):  # every sample clipped: a gradient of exactly 0
                assert (w == w0).all()
                continue
            worst = max(worst, gate(f"{name} d{kind}{l}", w - w0, w64 - w0, w32 - w0))
        if l == 0:  # the dropped observation entry
            assert (W[:, 17] == W0[:, 17]).all()
    return worst


GRAD_NETS = [((70, 33), 4, "tanh", True), ((70, 33), 10, "relu", False), ((), 4, "tanh", True), ((), 10, "relu", True),
             ((70, 33), 10, "tanh", True), ((70, 33), 4, "relu", True), ((256, 256, 256), 10, "tanh", True)]
GRAD_SEEDS = {((70, 33), 10, "tanh"): 6}  # the default seed puts a ratio 5e-5 from a clip boundary there (B = 33)
GRAD_BATCHES = {(256, 256, 256): ((130, 130),)}  # (B, n); the others:
GRAD_DEFAULT = ((1, 3), (17, 17), (33, 40), (40, 12))


@pytest.mark.parametrize("hidden,A,activation,bias", GRAD_NETS)
def test_gradients(envs, hidden, A, activation, bias):
    worst = 0.0
    for B, n in GRAD_BATCHES.get(hidden, GRAD_DEFAULT):
        spec, case = R.make_pg_case(hidden, A, activation, bias, n, seed=GRAD_SEEDS.get((hidden, A, activation), 5))
        worst = max(worst, pg_step_case(envs[A], spec, case, B, f"B={B} n={n}"))
    note(f"pg gradients {hidden} A={A} {activation}", worst)


EDGE_BATCHES = [1, 15, 16, 17, 31, 33, 513]


@pytest.mark.parametrize("B", EDGE_BATCHES)
def test_edge_batches(env, B):
    spec, case = R.make_pg_case((70, 33), 4, "tanh", True, B, seed=11)
    note(f"pg edge batches B={B}", pg_step_case(env, spec, case, B, f"B={B}"))


def test_ratios_spread_past_both_boundaries():
    """The cases above are worth their name: ratios on both sides of the clip range, and samples the clip removes."""
    spec, case = R.make_pg_case((70, 33), 4, "tanh", True, 513, seed=11)
    _, _, r = R.ratios(R.PgNet(spec, False).forward(case[0])[-1], case[1], case[2], case[4], False)
    assert (r < 1 - CLIP).mean() > 0.05 and (r > 1 + CLIP).mean() > 0.05 and ((r > 1 - CLIP) & (r < 1 + CLIP)).mean() > 0.05


# ------------------------------------------------------------------ 3. statistics and Adam over steps
ADAM = dict(steps=10, batch=64, lr=1e-3, seed=77)


def adam_case(activation):
    spec, case = R.make_pg_case((70, 33), 4, activation, True, 130 + 32, seed=21)
    held = case[0][130:]
    return spec, tuple(a[:130] for a in case[:4]) + (case[4],), held


@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_statistics_and_adam_over_steps(env, activation):
    spec, case, held = adam_case(activation)
    check = lambda net, idx: R.assert_clip_condition(net, case, idx, CLIP)  # noqa: E731
    s64, n64 = R.fit_pg(spec, case, ADAM["steps"], ADAM["batch"], False, clip=CLIP, seed=ADAM["seed"], lr=ADAM["lr"], on_batch=check)
    s32, n32 = R.fit_pg(spec, case, ADAM["steps"], ADAM["batch"], True, clip=CLIP, seed=ADAM["seed"], lr=ADAM["lr"])
    p = bind(spec, env)
    stats = p.fit_pg(*dev_case(case, env), ADAM["steps"], clip=CLIP, batch=ADAM["batch"], lr=ADAM["lr"], shuffle=True, seed=ADAM["seed"])
    out = p.eval(dev(held, env)).cpu().numpy()
    stats = stats.cpu().numpy()
    p.close()
    assert 0 < s64[:, 2].min() and s64[:, 2].max() < 1
    for c, name in enumerate(("loss", "kl", "clipped fraction")):
        note(f"pg adam {activation}: {name}", gate(name, stats[:, c], s64[:, c], s32[:, c]))
    note(f"pg adam {activation}: held-out outputs", gate("held-out outputs", out, n64.forward(held)[-1], n32.forward(held)[-1]))


# ------------------------------------------------------------------ 4. reproducibility, the shared optimiser state
def test_reproducible_and_shared_state(env):
    spec, case = R.make_pg_case((70, 33), 4, "tanh", True, 130, seed=31)
    target = FR.make_case((70, 33), 4, "tanh", True, 130, seed=31)[2]
    x = dev_case(case, env)
    y = dev(target, env)
    kw = dict(clip=CLIP, batch=64, lr=1e-3, shuffle=True, seed=5)
    a, b, c = bind(spec, env), bind(spec, env), bind(spec, env)
    sa, sb = a.fit_pg(*x, 6, **kw), b.fit_pg(*x, 6, **kw)
    sc = torch.cat([c.fit_pg(*x, 2, **kw), c.fit_pg(*x, 4, **kw)])
    wa = words(a.weights())
    assert (wa == words(b.weights())).all() and (bits(sa) == bits(sb)).all()
    assert (wa == words(c.weights())).all() and (bits(sa) == bits(sc)).all()
    assert (wa != words(spec_layers(spec))).any()
    s2 = b.fit_pg(*x, 6, **kw)  # the counter continues: other batches
    assert (s2.cpu().numpy() != sa.cpu().numpy()).any()
    b.load(spec_layers(spec))
    s3 = b.fit_pg(*x, 6, reset_optimizer=True, **kw)
    assert (bits(s3) == bits(sa)).all() and (words(b.weights()) == wa).all()
    # an MSE fit behind a PG fit continues t, m and v: the reference's sequence with one Net through both
    mse = dict(batch=64, lr=1e-3, shuffle=True, seed=5)
    la, lc = a.fit(x[0], y, 3, **mse), c.fit(x[0], y, 3, **mse)
    assert (bits(la) == bits(lc)).all()
    seqs = []
    for f32 in (False, True):
        check = None if f32 else (lambda net, idx: R.assert_clip_condition(net, case, idx, CLIP))
        _, net = R.fit_pg(spec, case, 6, 64, f32, clip=CLIP, seed=5, lr=1e-3, on_batch=check)
        net.__class__ = FR.Net  # the same weights, m, v and t under the MSE objective
        seqs.append(FR.fit(spec, case[0], target, 3, 64, f32, seed=5, k0=6, net=net, lr=1e-3)[0])
    note("mse losses behind a pg fit", gate("mse behind pg", la.cpu().numpy(), seqs[0], seqs[1]))
    fresh = bind(spec, env)
    fresh.load(a.weights())  # the same weights without the moments: another sequence
    a.load(c.weights())
    assert (bits(fresh.fit(x[0], y, 2, **mse)) != bits(a.fit(x[0], y, 2, **mse))).any()
    for p in (a, b, c, fresh):
        p.close()


# ------------------------------------------------------------------ 5. in place and ordered; set_log_std
def rollout_spec(log_std=-2.0):
    from mujoco_manip_amd.planner import action_box

    low, high = (np.array(v, F32) for v in action_box("abs_pos"))
    return make_spec(4, hidden=(64, 64), low=low, high=high, spread=1.4, obs_gain=4.0, log_std=np.full(4, log_std, F32))


@pytest.mark.parametrize("rows", [128, 192])
def test_in_place_and_ordered(rows):
    spec = rollout_spec()
    _, case = R.make_pg_case((), 4, "tanh", True, 130, seed=41)
    obs = case[0].copy()
    obs[:, 17] = 0.25
    names = RS.record_names() + ("mean", "noise")
    e1 = make_env(rows=rows)
    p1 = bind(spec, e1)
    x = [dev(a, e1) for a in (obs, case[1], case[2], case[3])]
    p1.fit_pg(*x, 5, clip=CLIP, batch=64, lr=1e-2, seed=3)  # no synchronise: eval and the rollout queue behind it
    mean1 = p1.eval(x[0])
    rec1 = e1.rollout_policy(p1, 8, record=names)
    layers = [(W.copy(), b.copy()) for W, b in p1.weights()]
    rec1, mean1, fin1 = RS.to_host(rec1), mean1.cpu().numpy(), RS.snapshot(e1)
    assert any((W != W0).any() for (W, _), (W0, _) in zip(layers, spec["layers"]))
    # set_log_std: the next rollout is the one of a policy created with that log_std, bit for bit: nothing else changed
    new = np.array([-1.0, -1.5, -0.5, -3.0], F32)
    p1.set_log_std(new)
    assert (p1.eval(x[0]).cpu().numpy() == mean1).all()
    rec1b, fin1b = RS.to_host(e1.rollout_policy(p1, 8, record=names, call=1)), RS.snapshot(e1)
    p1.close()
    e1.close()
    e2 = make_env(rows=rows)
    p2 = bind(dict(spec, layers=layers), e2)
    mean2 = p2.eval(dev(obs, e2)).cpu().numpy()
    rec2, fin2 = RS.to_host(e2.rollout_policy(p2, 8, record=names)), RS.snapshot(e2)
    p2.close()
    p3 = bind(dict(spec, layers=layers, log_std=new), e2)
    rec3, fin3 = RS.to_host(e2.rollout_policy(p3, 8, record=names, call=1)), RS.snapshot(e2)
    p3.close()
    e2.close()
    assert (mean1 == mean2).all()
    for name in rec1:
        assert (rec1[name] == rec2[name]).all(), name
        assert (rec1b[name] == rec3[name]).all(), name
    RS.assert_final(fin1, fin2)
    RS.assert_final(fin1b, fin3)
    # and the noise's scale is the new one: actions = clamp(mean + exp(new) z)
    want = np.clip(rec1b["mean"] + np.exp(new.astype(np.float64)).astype(F32) * rec1b["noise"], spec["low"], spec["high"])
    assert np.abs(rec1b["actions"] - want).max() <= 1e-6 and (rec1b["noise"] != 0).any()


# ------------------------------------------------------------------ 6. the critic
@pytest.mark.parametrize("rows", [128, 192])
def test_critic_on_returns(rows):
    from mujoco_manip_amd.policy import MlpCritic

    e = make_env(rows=rows, max_episode_steps=6)
    actor = bind(rollout_spec(), e)
    vspec = make_spec(1, hidden=(32,), seed=19)
    critic = MlpCritic(vspec["layers"], obs_shift=vspec["obs_shift"], obs_scale=vspec["obs_scale"]).bind(e)
    first = e._obs.clone()
    rec = e.rollout_policy(actor, 12, record=("obs", "reward", "done"))
    T, N = rec["reward"].shape
    obs = torch.cat([first[None], rec["obs"][:-1]]).reshape(-1, 85).contiguous()  # what each step was given
    value = critic.eval(obs).reshape(T, N)
    adv, ret = e.gae(rec["reward"], rec["done"], value, critic.eval(rec["obs"][-1])[:, 0].contiguous())
    obs_h, val_h, ret_h, done_h = obs.cpu().numpy(), value.cpu().numpy(), ret.cpu().numpy(), rec["done"].cpu().numpy()
    assert done_h[..., :2].any(), "the record holds no ended episode"
    v64, v32 = (FR.Net(vspec, f).forward(obs_h)[-1].reshape(T, N) for f in (False, True))
    note(f"critic eval rows={rows}", gate("critic eval", val_h, v64, v32))
    r64, r32 = (R.gae(rec["reward"].cpu().numpy(), done_h, val_h, critic.eval(rec["obs"][-1])[:, 0].cpu().numpy(), 0.99, 0.95, f)[1]
                for f in (False, True))
    note(f"critic returns rows={rows}", gate("returns", ret_h, r64, r32))
    loss = critic.fit(obs, ret.reshape(-1, 1).contiguous(), 30, batch=64, lr=3e-3, seed=2).cpu().numpy()
    assert np.isfinite(loss).all() and loss[-5:].mean() < loss[:5].mean(), loss
    for p in (actor, critic):
        p.close()
    e.close()


# ------------------------------------------------------------------ 7. refusals
def test_einval_touches_nothing(env):
    from mujoco_manip_amd import _lib

    spec, case = R.make_pg_case((70, 33), 4, "tanh", True, 40, seed=51)
    p = bind(spec, env)
    x = dev_case(case, env)
    p.fit_pg(*x, 2, clip=CLIP, batch=16)  # a fitted policy with optimiser state
    before = p.eval(x[0]).cpu().numpy()
    w_before = p.weights()
    d, L = p.device_policy, p.device_policy.L
    stats = torch.full((4, 3), -7.0, device=env.device)
    ptrs = dict(obs=x[0].data_ptr(), mean_old=x[1].data_ptr(), noise=x[2].data_ptr(), adv=x[3].data_ptr())

    def call(ptr=d.ptr, n=40, steps=2, null_cfg=False, clip=CLIP, null=(), **kw):
        c = dict(optimizer=1, batch=16, shuffle=1, reset_optimizer=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=1)
        c.update(kw)
        cfg = _lib.MMXPgConfig(fit=_lib.MMXFitConfig(**c), clip=clip)
        a = [None if k in null else C.c_void_p(v) for k, v in ptrs.items()]
        return L.mmx_policy_fit_pg(ptr, *a, n, steps, None if null_cfg else C.byref(cfg), C.c_void_p(stats.data_ptr()))

    nan, inf = float("nan"), float("inf")
    cases = [dict(ptr=None), dict(null=("obs",)), dict(null=("mean_old",)), dict(null=("noise",)), dict(null=("adv",)), dict(null_cfg=True),
             dict(n=0), dict(n=-3), dict(n=2**31), dict(steps=-1), dict(batch=0), dict(batch=-1), dict(batch=65537), dict(optimizer=2),
             dict(optimizer=-1), dict(lr=0.0), dict(lr=-1.0), dict(lr=nan), dict(lr=inf), dict(eps=0.0), dict(eps=nan), dict(eps=inf),
             dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan), dict(beta2=1.0), dict(beta2=-0.1), dict(beta2=nan),
             dict(clip=0.0), dict(clip=1.0), dict(clip=-0.2), dict(clip=1.5), dict(clip=nan), dict(clip=inf)]
    for kw in cases:
        assert call(**kw) == -1, kw  # MMX_EINVAL
        assert (p.eval(x[0]).cpu().numpy() == before).all(), kw
    assert call(steps=0, reset_optimizer=0) == 0  # nothing to do, and nothing done
    assert (stats.cpu().numpy() == -7.0).all()
    # a deterministic policy has no ratio: created without log_std, or with a std of 0 (exp underflows)
    for log_std in (None, np.array([0, 0, -1000, 0], F32)):
        q = bind(dict(spec, log_std=log_std), env)
        assert call(ptr=q.device_policy.ptr) == -1
        assert all((W == W0).all() for (W, _), (W0, _) in zip(q.weights(), spec["layers"]))
        assert L.mmx_policy_set_log_std(q.device_policy.ptr, np.zeros(4, F32).ctypes.data_as(C.POINTER(C.c_float))) == 0
        assert call(ptr=q.device_policy.ptr) == 0  # with a std it has one
        q.close()
    bad = np.array([0, nan, 0, 0], F32)
    assert L.mmx_policy_set_log_std(d.ptr, None) == -1 and L.mmx_policy_set_log_std(d.ptr, bad.ctypes.data_as(C.POINTER(C.c_float))) == -1
    for (W, b), (W0, b0) in zip(p.weights(), w_before):
        assert (W == W0).all() and (b == b0).all()
    # the optimiser state was not reset by a refused call: the next steps continue as those of an undisturbed twin
    q = bind(spec, env)
    q.fit_pg(*x, 2, clip=CLIP, batch=16)
    assert (bits(q.fit_pg(*x, 3, clip=CLIP, batch=16)) == bits(p.fit_pg(*x, 3, clip=CLIP, batch=16))).all()
    p.close()
    q.close()
    # mmx_gae
    T, N = 3, 5
    reward, done, value, value_last = R.make_gae_case(T, N)
    g = [dev(reward, env), dev(done, env, np.int32), dev(value, env), dev(value_last, env)]
    out = [torch.full((T, N), -7.0, device=env.device) for _ in range(2)]
    sim = env.sim

    def gae(sim_ptr=sim.ptr, T=T, N=N, gamma=0.99, lam=0.95, null=(), null_cfg=False):
        cfg = _lib.MMXGaeConfig(gamma=gamma, lambda_=lam, normalize=1)
        a = [None if i in null else C.c_void_p(t.data_ptr()) for i, t in enumerate(g + out)]
        return sim.L.mmx_gae(sim_ptr, None if null_cfg else C.byref(cfg), T, N, *a)

    for kw in [dict(sim_ptr=None), dict(null_cfg=True), dict(null=(0,)), dict(null=(1,)), dict(null=(2,)), dict(null=(3,)), dict(null=(4,)),
               dict(T=-1), dict(N=0), dict(N=-2), dict(gamma=1.5), dict(gamma=-0.1), dict(gamma=nan), dict(gamma=inf), dict(lam=1.01),
               dict(lam=-0.5), dict(lam=nan)]:
        assert gae(**kw) == -1, kw
    assert gae(T=0) == 0
    env.synchronize()
    assert all((o.cpu().numpy() == -7.0).all() for o in out)
    assert gae(null=(5,)) == 0  # ret_out may be NULL
    env.synchronize()
    assert (out[0].cpu().numpy() != -7.0).all() and (out[1].cpu().numpy() == -7.0).all()


# ------------------------------------------------------------------ 8. direction
def direction_case():
    spec, case = R.make_pg_case((70, 33), 4, "tanh", True, 96, seed=61)
    obs, _, noise, _, std = case
    mean_old = R.PgNet(spec, False).forward(obs)[-1].astype(F32)  # on-policy: the ratios start at 1
    adv = np.where(noise[:, 0] > 0, 1.0, -1.0).astype(F32)
    return spec, (obs, mean_old, noise, adv, std)


DIRECTION = dict(steps=20, batch=96, lr=1e-3, shuffle=False)


def test_direction(env):
    spec, case = direction_case()
    obs = case[0]
    before64 = R.PgNet(spec, False).forward(obs)[-1][:, 0].mean()
    _, n64 = R.fit_pg(spec, case, DIRECTION["steps"], DIRECTION["batch"], False, clip=CLIP, shuffle=False, lr=DIRECTION["lr"])
    rise64 = n64.forward(obs)[-1][:, 0].mean() - before64
    assert rise64 > 0, "the fp64 reference does not rise: the case is wrong"
    p = bind(spec, env)
    x = dev_case(case, env)
    before = p.eval(x[0])[:, 0].mean().item()
    stats = p.fit_pg(*x, DIRECTION["steps"], clip=CLIP, **{k: v for k, v in DIRECTION.items() if k != "steps"}).cpu().numpy()
    rise = p.eval(x[0])[:, 0].mean().item() - before
    p.close()
    print(f"direction: component 0's mean rose by {rise:.4g} (fp64 reference {rise64:.4g}); loss {stats[0, 0]:.4g} -> {stats[-1, 0]:.4g}")
    assert rise > 0
