"""Fitting the MLP policy on the device (mmx_policy_fit, mmx_policy_get_weights, mmx_policy_set_weights;
MlpPolicy.fit / weights / load).

The error measure of a tensor T against the fp64 restatement T64 (tests/policy_fit_ref.py) is
err(T) = max |T - T64| / max |T64|, and the gate is err_gpu <= 8 max(err_yardstick, 2^-24) per tensor: the yardstick
is the same computation with every multiply-add rounded to fp32 in index order, on the same case.  The factor 8 is
the project's precedent (contact forces): it covers a different summation order (tiles of 16 samples, K chunks of
512) and the hardware exp2 and reciprocal in tanh (8 * 2^-24 absolute).  Every test prints its worst fraction of the
gate; MMX_FIT_MARGINS=<path> collects them.

1. gradients: one SGD step at lr = 1, shuffle = 0, B = n, so the exported weight change is the gradient;
2. edge tiles: every B around the sample tile (16), the GEMM's staging block (32) and K chunk (512), and the 64 x 64
   output tile, for 85-70-33-4;
3. Adam over ten shuffled steps: the loss sequence and the fitted network's outputs on held-out observations;
4. reproducibility, bit for bit: two policies alike, 6 steps = 2 + 4 steps, reset_optimizer;
5. in place and ordered: eval and a rollout queued right behind fit run the new weights;
6. invisible otherwise: an export and re-set changes no bit of a DAgger rollout;
7. every MMX_EINVAL case, with the policy untouched;
8. the DAgger fit end to end, small."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import policy_fit_ref as R
from policy_ref import make_spec
import rollout_support as RS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
# tests/test_traj_rollout.py's envs
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
    """The sims whose streams the policies of the sim-less tests are fitted on, by action dimension (a policy binds
    to an env of its own action width: abs_pos has 4, the relative 6D mode 10)."""
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


def dev(a, env):
    return torch.as_tensor(np.ascontiguousarray(a, F32), device=env.device)


def gate(name, got, want64, yard):
    """Asserts err(got) <= 8 max(err(yard), 2^-24); returns the fraction of the gate."""
    e, y = R.err(got, want64), R.err(yard, want64)
    frac = e / (8 * max(y, R.U))
    assert frac <= 1.0, f"{name}: err {e:.3e}, yardstick {y:.3e}, {frac:.2f} of the gate"
    return frac


def spec_layers(spec):
    return [(W, np.zeros(W.shape[0], F32) if b is None else b) for W, b in spec["layers"]]


def sgd_step_case(env, spec, obs, target, name):
    """One SGD step at lr = 1 on the whole set in order: the exported weight change against the fp64 gradient."""
    B = len(obs)
    p = bind(spec, env)
    loss = p.fit(dev(obs, env), dev(target, env), 1, batch=B, lr=1.0, optimizer="sgd", shuffle=False)
    after = p.weights()
    loss = loss.cpu().numpy()
    p.close()
    n64, n32 = R.Net(spec, False), R.Net(spec, True)
    l64, l32 = n64.step(obs, target, "sgd", lr=1.0), n32.step(obs, target, "sgd", lr=1.0)
    worst = gate(f"{name} loss", loss, [l64], [l32])
    for l, ((W0, b0), (W, b), (W64, b64), (W32, b32)) in enumerate(zip(spec_layers(spec), after, n64.layers, n32.layers)):
        for kind, w0, w, w64, w32 in (("W", W0, W, W64, W32), ("b", b0, b, b64, b32)):
            w0 = w0.astype(np.float64)
            worst = max(worst, gate(f"{name} d{kind}{l}", w - w0, w64 - w0, w32 - w0))
        if l == 0:  # the dropped observation entry
            assert (W[:, 17] == W0[:, 17]).all()
    return worst


# ------------------------------------------------------------------ 1. gradients
@pytest.mark.parametrize("hidden,A,activation,bias", R.GRAD_CASES + [((256, 256, 256), 10, "tanh", True)])
def test_gradients(envs, hidden, A, activation, bias):
    worst, env = 0.0, envs[A]
    for B in ((130,) if hidden == (256, 256, 256) else (1, 63, 65)):
        spec, obs, target = R.make_case(hidden, A, activation, bias, B)
        worst = max(worst, sgd_step_case(env, spec, obs, target, f"B={B}"))
    note(f"gradients {hidden} A={A} {activation}", worst)


# ------------------------------------------------------------------ 2. edge tiles
@pytest.mark.parametrize("B", [1, 15, 16, 17, 31, 32, 33, 63, 65, 130, 511, 512, 513])
def test_edge_tiles(env, B):
    spec, obs, target = R.make_case((70, 33), 4, "tanh", True, B, seed=11)
    note(f"edge tiles B={B}", sgd_step_case(env, spec, obs, target, f"B={B}"))


# ------------------------------------------------------------------ 3. Adam over steps
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_adam_over_steps(env, activation):
    spec, obs, target = R.make_case((70, 33), 4, activation, True, 130 + 32, seed=21)
    held, obs, target = obs[130:], obs[:130], target[:130]
    p = bind(spec, env)
    loss = p.fit(dev(obs, env), dev(target, env), 10, batch=64, lr=1e-3, shuffle=True, seed=77)
    out = p.eval(dev(held, env)).cpu().numpy()
    loss = loss.cpu().numpy()
    p.close()
    (l64, n64), (l32, n32) = (R.fit(spec, obs, target, 10, 64, f32, seed=77, lr=1e-3) for f32 in (False, True))
    a = gate("loss sequence", loss, l64, l32)
    b = gate("held-out outputs", out, n64.forward(held)[-1], n32.forward(held)[-1])
    assert loss[-1] < loss[0]
    note(f"adam {activation}: losses", a)
    note(f"adam {activation}: held-out outputs", b)


# ------------------------------------------------------------------ 4. reproducibility
def test_reproducible(env):
    spec, obs, target = R.make_case((70, 33), 4, "tanh", True, 130, seed=31)
    x, y = dev(obs, env), dev(target, env)
    kw = dict(batch=64, lr=1e-3, shuffle=True, seed=5)

    def words(layers):
        return np.concatenate([np.concatenate([W.ravel(), b.ravel()]) for W, b in layers]).view(np.uint32)

    a, b, c = bind(spec, env), bind(spec, env), bind(spec, env)
    la, lb = a.fit(x, y, 6, **kw), b.fit(x, y, 6, **kw)
    lc = torch.cat([c.fit(x, y, 2, **kw), c.fit(x, y, 4, **kw)])
    wa = words(a.weights())
    assert (wa == words(b.weights())).all() and (la.cpu().numpy().view(np.uint32) == lb.cpu().numpy().view(np.uint32)).all()
    assert (wa == words(c.weights())).all() and (la.cpu().numpy().view(np.uint32) == lc.cpu().numpy().view(np.uint32)).all()
    assert (wa != words(spec_layers(spec))).any()
    # the counter continues: 6 more steps are not the first 6; reset_optimizer from the first weights is
    l2 = b.fit(x, y, 6, **kw)
    assert (l2.cpu().numpy() != la.cpu().numpy()).any()
    b.load(spec_layers(spec))
    l3 = b.fit(x, y, 6, reset_optimizer=True, **kw)
    assert (l3.cpu().numpy().view(np.uint32) == la.cpu().numpy().view(np.uint32)).all() and (words(b.weights()) == wa).all()
    # a larger batch grows the workspace behind queued work; then the small batch again
    big = c.fit(x, y, 2, batch=600, lr=1e-3, shuffle=True, seed=5)
    assert np.isfinite(big.cpu().numpy()).all() and np.isfinite(c.fit(x, y, 1, **kw).cpu().numpy()).all()
    for p in (a, b, c):
        p.close()


# ------------------------------------------------------------------ 5. in place and ordered
def rollout_spec(hidden=(64, 64)):
    from mujoco_manip_amd.planner import action_box

    low, high = (np.array(v, F32) for v in action_box("abs_pos"))
    return make_spec(4, hidden=hidden, low=low, high=high, spread=1.4, obs_gain=4.0)


@pytest.mark.parametrize("rows", [128, 192])
def test_in_place_and_ordered(rows):
    spec = rollout_spec()
    _, obs, _ = R.make_case((), 4, "tanh", True, 130, seed=41)
    obs[:, 17] = 0.25
    target = np.random.default_rng(4).uniform(spec["low"], spec["high"], (130, 4)).astype(F32)
    e1 = make_env(rows=rows)
    p1 = bind(spec, e1)
    x = dev(obs, e1)
    p1.fit(x, dev(target, e1), 5, batch=64, lr=1e-2, seed=3)  # no synchronise: eval and the rollout queue behind it
    mean1 = p1.eval(x)
    rec1 = e1.rollout_policy(p1, 8, record=RS.record_names() + ("mean",))
    layers = [(W.copy(), b.copy()) for W, b in p1.weights()]
    rec1, mean1, fin1 = RS.to_host(rec1), mean1.cpu().numpy(), RS.snapshot(e1)
    assert any((W != W0).any() for (W, _), (W0, _) in zip(layers, spec["layers"]))
    p1.load(layers)  # set_weights(get_weights()): no bit of the blob's behaviour changes
    assert (p1.eval(x).cpu().numpy() == mean1).all()
    p1.close()
    e1.close()
    e2 = make_env(rows=rows)
    p2 = bind(dict(spec, layers=layers), e2)
    mean2 = p2.eval(dev(obs, e2)).cpu().numpy()
    rec2 = RS.to_host(e2.rollout_policy(p2, 8, record=RS.record_names() + ("mean",)))
    fin2 = RS.snapshot(e2)
    p2.close()
    e2.close()
    assert (mean1 == mean2).all()
    for name in rec1:
        assert (rec1[name] == rec2[name]).all(), name
    RS.assert_final(fin1, fin2)


# ------------------------------------------------------------------ 6. invisible otherwise
@pytest.mark.parametrize("rows", [128, 192])
def test_export_and_reset_are_invisible(rows):
    spec = dict(rollout_spec(), log_std=np.full(4, np.log(0.05), F32))
    recs, fins = [], []
    for reset in (False, True):
        e = make_env(rows=rows)
        p = bind(spec, e)
        if reset:
            p.load(p.weights())
        recs.append(RS.to_host(e.rollout_dagger(p, 8, beta=0.5, call=2)))
        fins.append(RS.snapshot(e))
        p.close()
        e.close()
    for name in recs[0]:
        assert (recs[0][name] == recs[1][name]).all(), name
    RS.assert_final(fins[0], fins[1])


# ------------------------------------------------------------------ 7. refusals
def test_einval_touches_nothing(env):
    from mujoco_manip_amd import _lib

    spec, obs, target = R.make_case((70, 33), 4, "tanh", True, 40, seed=51)
    p = bind(spec, env)
    x, y = dev(obs, env), dev(target, env)
    p.fit(x, y, 2, batch=16)  # a fitted policy with optimiser state
    before = p.eval(x).cpu().numpy()
    w_before = p.weights()
    d, L = p.device_policy, p.device_policy.L
    loss = torch.full((4,), -7.0, device=env.device)

    def call(ptr=d.ptr, obs_ptr=x.data_ptr(), tgt_ptr=y.data_ptr(), n=40, steps=2, null_cfg=False, **kw):
        c = dict(optimizer=1, batch=16, shuffle=1, reset_optimizer=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=1)
        c.update(kw)
        cfg = _lib.MMXFitConfig(**c)
        return L.mmx_policy_fit(ptr, C.c_void_p(obs_ptr) if obs_ptr else None, C.c_void_p(tgt_ptr) if tgt_ptr else None, n, steps,
                                None if null_cfg else C.byref(cfg), C.c_void_p(loss.data_ptr()))

    nan, inf = float("nan"), float("inf")
    cases = [dict(ptr=None), dict(obs_ptr=0), dict(tgt_ptr=0), dict(null_cfg=True), dict(n=0), dict(n=-3), dict(n=2**31), dict(steps=-1),
             dict(batch=0), dict(batch=-1), dict(batch=65537), dict(optimizer=2), dict(optimizer=-1), dict(lr=0.0), dict(lr=-1.0),
             dict(lr=nan), dict(lr=inf), dict(eps=0.0), dict(eps=nan), dict(eps=inf), dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan),
             dict(beta2=1.0), dict(beta2=-0.1), dict(beta2=nan)]
    for kw in cases:
        assert call(**kw) == -1, kw  # MMX_EINVAL
        assert (p.eval(x).cpu().numpy() == before).all(), kw
    assert call(steps=0, reset_optimizer=0) == 0  # nothing to do, and nothing done
    assert (loss.cpu().numpy() == -7.0).all()
    for (W, b), (W0, b0) in zip(p.weights(), w_before):
        assert (W == W0).all() and (b == b0).all()
    # the optimiser state was not reset by a refused call: the next steps continue as those of an undisturbed twin
    q = bind(spec, env)
    q.fit(x, y, 2, batch=16)
    assert (q.fit(x, y, 3, batch=16).cpu().numpy() == p.fit(x, y, 3, batch=16).cpu().numpy()).all()
    assert L.mmx_policy_get_weights(None, None, None) == -1 and L.mmx_policy_set_weights(d.ptr, None, None) == -1
    p.close()
    q.close()


# ------------------------------------------------------------------ 8. end to end, small
@pytest.mark.parametrize("rows", [128, 192])
def test_dagger_fit_end_to_end(rows):
    e = make_env(n=64, rows=rows, max_episode_steps=50)
    spec = rollout_spec()
    p = bind(spec, e)
    rec = e.rollout_dagger(p, 40, beta=1.0, record=("obs_in", "expert_action"))  # the expert acts and labels
    x, y = rec["obs_in"].reshape(-1, 85).contiguous(), rec["expert_action"].reshape(-1, 4).contiguous()
    loss = p.fit(x, y, 50, batch=128, lr=1e-3, seed=9).cpu().numpy()
    p.close()
    e.close()
    obs, target = x.cpu().numpy(), y.cpu().numpy()
    assert obs.shape == (2560, 85) and loss[-1] < loss[0]
    (l64, _), (l32, _) = (R.fit(spec, obs, target, 50, 128, f32, seed=9, lr=1e-3) for f32 in (False, True))
    note(f"end to end rows={rows}: final loss", gate("final loss", loss[-1:], l64[-1:], l32[-1:]))
    note(f"end to end rows={rows}: loss sequence", gate("loss sequence", loss, l64, l32))
