"""Restatements of generalised advantage estimation and of the policy-gradient step (include/mmx_api.h,
"Policy-gradient fits on the device"; csrc/mmx_pg.h) for tests/test_pg_host.py (CPU) and tests/test_pg.py (GPU).

As in tests/policy_fit_ref.py, whose Net, error measure, batch indices and seeded cases are imported: one code path,
two arithmetics.  `f32=False` is the fp64 restatement, `f32=True` the yardstick with every operation rounded to fp32
in index order (exp correctly rounded).  Added here: PPO's output delta and its three statistics (PgNet.gradients;
Net.step then applies SGD or Adam unchanged), GAE, the advantages' normalisation, the condition every PPO case has to
meet (no ratio near a clip boundary, no advantage 0), and the seeded cases."""
import numpy as np

from policy_fit_ref import F32, F64, U, Net, _fma, batch_indices, err, make_case  # noqa: F401

NORM_EPS = 1e-8
CLIP_MARGIN = 1e-4  # relative distance every ratio keeps from 1 - clip and 1 + clip in the fp64 reference


# ------------------------------------------------------------------ GAE
def gae(reward, done, value, value_last, gamma, lam, f32):
    """(adv, ret) [T, N]; gamma, lam and their product taken at their fp32 values (the device gets floats)."""
    dt = F32 if f32 else F64
    T, N = reward.shape
    gamma, gl = F32(gamma), F32(F32(gamma) * F32(lam))
    r, v, vl = reward.astype(dt), value.astype(dt), value_last.astype(dt)
    adv, ret = np.zeros((T, N), dt), np.zeros((T, N), dt)
    nxt = np.zeros(N, dt)
    for t in range(T - 1, -1, -1):
        end = (done[t, :, 0] != 0) | (done[t, :, 1] != 0)
        nv = np.where(end, 0, vl if t == T - 1 else v[t + 1]).astype(dt)
        delta = (_fma(gamma, nv, r[t], f32) - v[t]).astype(dt)
        nxt = np.where(end, delta, _fma(gl, nxt, delta, f32)).astype(dt)
        adv[t], ret[t] = nxt, (nxt + v[t]).astype(dt)
    return adv, ret


def normalise(adv, f32):
    """(adv - mean) / (sqrt(var) + 1e-8) over all entries; the yardstick sums one fp32 chain in index order."""
    x = adv.ravel()
    if not f32:
        x = x.astype(F64)
        return ((x - x.mean()) / (np.sqrt(((x - x.mean()) ** 2).mean()) + NORM_EPS)).reshape(adv.shape)
    x = x.astype(F32)
    n = F32(x.size)
    mean = F32(np.cumsum(x, dtype=F32)[-1] / n)
    c = (x - mean).astype(F32)
    var = F32(np.cumsum((c * c).astype(F32), dtype=F32)[-1] / n)
    return (c / F32(np.sqrt(var) + F32(NORM_EPS))).astype(F32).reshape(adv.shape)


# ------------------------------------------------------------------ PPO's clipped surrogate
def ratios(mean, mean_old, noise, std, f32):
    """(z', log r, r) of samples [B, A]: the density ratio of the pre-clamp sample u = mean_old + std z."""
    dt = F32 if f32 else F64
    z, sd = noise.astype(dt), std.astype(dt)
    u = _fma(sd[None, :], z, mean_old.astype(dt), f32).astype(dt)
    zn = ((u - mean.astype(dt)).astype(dt) / sd[None, :]).astype(dt)
    lr = np.zeros(len(z), dt)
    for a in range(z.shape[1]):  # a ascending
        dd = _fma(-zn[:, a], zn[:, a], (z[:, a] * z[:, a]).astype(dt), f32)
        lr = _fma(0.5, dd, lr, f32).astype(dt)
    r = np.exp(lr.astype(F64)).astype(dt)
    return zn, lr, r


class PgNet(Net):
    """Net with PPO's objective: gradients(obs, pack) takes pack = (mean_old [B, A], noise [B, A], adv [B], std [A],
    clip) where Net.gradients takes the targets, and returns the three statistics where it returns the loss, so
    Net.step (the optimisers) serves unchanged."""

    def gradients(self, obs, pack):
        mean_old, noise, adv, std, clip = pack
        dt, f32 = self.dt, self.f32
        xs = self.forward(obs)
        B = len(obs)
        zn, lr, r = ratios(xs[-1], mean_old, noise, std, f32)
        adv = adv.astype(dt)
        lo, hi = (F32(1) - F32(clip), F32(1) + F32(clip))
        lo, hi = (lo, hi) if f32 else (F64(lo), F64(hi))
        invB = F32(1) / F32(B) if f32 else 1.0 / B
        live = ~(((adv > 0) & (r > hi)) | ((adv < 0) & (r < lo)))
        loss_s = -np.minimum((r * adv).astype(dt), (np.clip(r, lo, hi) * adv).astype(dt))
        kl_s = ((r - 1).astype(dt) - lr).astype(dt)
        cols = (loss_s, kl_s, (~live).astype(dt))
        if f32:  # one fp32 chain per statistic, samples in order
            stats = np.array([F32(np.cumsum(c, dtype=F32)[-1] * invB) for c in cols], F32)
        else:
            stats = np.array([c.sum() * invB for c in cols], F64)
        g = np.where(live, ((invB * adv).astype(dt) * r).astype(dt), 0).astype(dt)
        d = (-(g[:, None] * (zn / std.astype(dt)[None, :]).astype(dt))).astype(dt)
        return stats, self.backward(xs, d)

    def backward(self, xs, d):
        """[(dW, db)] from the output delta d [B, A]: the loops of Net.gradients (the batch in index order)."""
        dt, f32, B = self.dt, self.f32, len(d)
        grads = [None] * len(self.layers)
        for l in range(len(self.layers) - 1, -1, -1):
            x = xs[l]
            dW, db = np.zeros_like(self.layers[l][0]), np.zeros_like(self.layers[l][1])
            for s in range(B):
                dW = _fma(d[s][:, None], x[s][None, :], dW, f32)
                db = _fma(1.0, d[s], db, f32)
            grads[l] = (dW.astype(dt), db.astype(dt))
            if l:
                W = self.layers[l][0]
                back = np.zeros((B, W.shape[1]), dt)
                for j in range(W.shape[0]):
                    back = _fma(d[:, j:j + 1], W[j][None, :], back, f32)
                a = xs[l]
                grad = _fma(-a, a, 1.0, f32) if self.activation == "tanh" else (a > 0).astype(dt)
                d = (back.astype(dt) * grad.astype(dt)).astype(dt)
        return grads


def fit_pg(spec, case, steps, batch, f32, clip=0.2, optimizer="adam", shuffle=True, seed=0, k0=0, net=None, on_batch=None, **opt):
    """`steps` PG steps from step counter k0 on case = (obs, mean_old, noise, adv, std); returns (stats [steps, 3],
    net).  on_batch(net, idx): called before every step (the clip condition's check)."""
    obs, mean_old, noise, adv, std = case
    net = PgNet(spec, f32) if net is None else net
    net.t = k0
    stats = []
    for k in range(k0, k0 + steps):
        idx = batch_indices(shuffle, seed, k, batch, len(obs))
        if on_batch:
            on_batch(net, idx)
        stats.append(net.step(obs[idx], (mean_old[idx], noise[idx], adv[idx], std, clip), optimizer, **opt))
    return np.array(stats), net


def clip_margin(net64, case, idx, clip):
    """The smallest relative distance of a sample's fp64 ratio from either clip boundary, over the batch idx."""
    obs, mean_old, noise, adv, std = case
    _, _, r = ratios(net64.forward(obs[idx])[-1], mean_old[idx], noise[idx], std, False)
    lo, hi = F64(F32(1) - F32(clip)), F64(F32(1) + F32(clip))
    return float(min(np.abs(r / lo - 1).min(), np.abs(r / hi - 1).min()))


def assert_clip_condition(net64, case, idx, clip):
    """The condition on a PPO case's inputs, on the fp64 reference alone: the clip test is discontinuous, so no
    sample's ratio may lie within CLIP_MARGIN (relative) of 1 - clip or 1 + clip, and no advantage may be 0."""
    assert (case[3][idx] != 0).all(), "an advantage is 0"
    m = clip_margin(net64, case, idx, clip)
    assert m > CLIP_MARGIN, f"a ratio lies within {m:.2e} of a clip boundary: choose another seed"


# ------------------------------------------------------------------ the shared cases
def make_pg_case(hidden, A, activation, bias, n, seed=5, perturb=0.15, sigma=(0.5, 1.0)):
    """A seeded policy (make_case's) with a log_std, and n samples of a rollout under a perturbed copy of it:
    mean_old = the copy's output, so the ratios spread to both sides of the clip range; noise ~ N(0, 1); advantages
    ~ N(0, 1), none 0.  Returns (spec, (obs, mean_old, noise, adv, std)).

    sigma: the range std is drawn from.  The output delta is (u - mean') / std^2 times the sample's weight, so an
    absolute error e of the forward pass's mean (the device's tanh is allowed 8 * 2^-24 absolute, and the yardstick's
    is correctly rounded) reaches the gradient as e / (std |z'|) relative, where the mean-squared error's delta
    mean - y carries it as e / |mean - y|, |mean - y| ~ 0.3 in make_case.  std in 0.5 .. 1 keeps std |z'| of a typical
    draw at that size, so the same gate measures the same thing; it is also where a log_std schedule starts.
    perturb: the relative size of the copy's weight noise.  Besides spreading the ratios past both clip boundaries it
    sets the size of log r, and with it the conditioning of the KL statistic: (r - 1) - log r is about (log r)^2 / 2
    and carries the rounding of r itself, 2^-24 r absolute per sample, so log r has to be a few tenths for fp32 to
    give the statistic to a few units of 2^-24 at all."""
    spec, obs, _ = make_case(hidden, A, activation, bias, n, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    log_std = np.log(rng.uniform(sigma[0], sigma[1], A)).astype(F32)
    spec = dict(spec, log_std=log_std, low=None, high=None)
    old = dict(spec, layers=[(W + (perturb * rng.standard_normal(W.shape) * np.abs(W).mean()).astype(F32),
                              None if b is None else b + (perturb * rng.standard_normal(b.shape)).astype(F32))
                             for W, b in spec["layers"]])
    mean_old = Net(old, False).forward(obs)[-1].astype(F32)
    noise = rng.standard_normal((n, A)).astype(F32)
    adv = rng.standard_normal(n).astype(F32)
    adv[adv == 0] = F32(0.5)
    std = np.exp(log_std.astype(F64)).astype(F32)
    return spec, (obs, mean_old, noise, adv, std)


GAE_SHAPES = [(1, 1), (5, 63), (5, 65), (7, 130)]


def make_gae_case(T, N, seed=3):
    """Seeded rewards and values, and done patterns: terminations at t = 0, at t = T - 1 and mid-way, a truncation,
    both flags on one step (as far as the shape has room), and sparse random ends elsewhere."""
    rng = np.random.default_rng(seed + 31 * T + N)
    reward = rng.uniform(-1, 2, (T, N)).astype(F32)
    value = rng.uniform(-3, 3, (T, N)).astype(F32)
    value_last = rng.uniform(-3, 3, N).astype(F32)
    done = np.zeros((T, N, 3), np.int32)
    done[..., 0] = rng.random((T, N)) < 0.08
    done[..., 1] = rng.random((T, N)) < 0.08
    done[0, 0, 0] = 1                # a termination at t = 0
    if N > 1:
        done[:, 1] = 0
        done[T - 1, 1, 0] = 1        # at t = T - 1
    if N > 4:
        done[:, 2:5] = 0
        done[T // 2, 2, 0] = 1       # mid-way
        done[T // 2, 3, 1] = 1       # a truncation
        done[T // 2, 4, :2] = 1      # both flags on one step
    done[..., 2] = done[..., 0] & (rng.random((T, N)) < 0.5)
    return reward, done, value, value_last
