"""Restatements of the policy's training step (include/mmx_api.h, "Fitting a policy on the device";
csrc/mmx_policy_fit.h) for tests/test_policy_fit_host.py (CPU) and tests/test_policy_fit.py (GPU).

One code path, two arithmetics.  `f32=False` is the fp64 restatement: loss, gradients, SGD and Adam in double.
`f32=True` is the yardstick: the same computation with every multiply-add rounded to fp32 in index order (a fused
multiply-add is emulated as the fp64 product and sum rounded once to fp32: the product of two fp32 values is exact
in fp64, so only the rare double rounding of the sum differs from a true fma), tanh correctly rounded.  The
yardstick shows what error fp32 arithmetic itself gives on a case, which is what a gate on the device's error is
measured against: err(T) = max |T - T64| / max |T64|.

Also here: the batch's pair indices (sequential and Philox4x32-10), Adam's update in the stated operation order
bit for bit, and the seeded cases the two test files share."""
import numpy as np

from policy_ref import make_spec

F32, F64 = np.float32, np.float64
FIT_DOMAIN = 0xF17BA7C4
U = 2.0 ** -24


# ------------------------------------------------------------------ the batch's pair indices
def philox4x32_10(ctr, key):
    c, k = [int(v) for v in ctr], [int(v) for v in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def batch_indices(shuffle, seed, k, B, n):
    """The pairs of optimisation step k (the policy's running counter, from 0)."""
    if not shuffle:
        return np.array([(k * B + s) % n for s in range(B)], np.int64)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = []
    for s in range(B):
        x = philox4x32_10((k & 0xFFFFFFFF, (k >> 32) & 0xFFFFFFFF, s // 4, FIT_DOMAIN), key)[s % 4]
        out.append((x * n) >> 32)
    return np.array(out, np.int64)


# ------------------------------------------------------------------ the two arithmetics
def _fma(a, b, c, f32):
    r = np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)
    return r.astype(F32) if f32 else r


def err(T, T64):
    """max |T - T64| / max |T64| (0 / 0 = 0)."""
    T64 = np.asarray(T64, F64)
    d, s = np.abs(np.asarray(T, F64) - T64).max(), np.abs(T64).max()
    return 0.0 if d == 0 else d / s


class Net:
    """The trained part of a policy in one arithmetic: layers [(W [out, in], b [out])], torch layout."""

    def __init__(self, spec, f32):
        self.f32, self.dt = f32, F32 if f32 else F64
        self.activation = spec["activation"]
        self.shift, self.scale = spec["obs_shift"].astype(self.dt), spec["obs_scale"].astype(self.dt)
        self.layers = [(W.astype(self.dt), (np.zeros(W.shape[0]) if b is None else b).astype(self.dt)) for W, b in spec["layers"]]
        self.m = [(np.zeros_like(W), np.zeros_like(b)) for W, b in self.layers]
        self.v = [(np.zeros_like(W), np.zeros_like(b)) for W, b in self.layers]
        self.t = 0

    def forward(self, obs):
        """[x_0, x_1, .., mean]: every layer's input and the output, of obs [B, 85] (float32 values)."""
        x = (obs.astype(self.dt) - self.shift) * self.scale  # two roundings in fp32
        xs = [x]
        for l, (W, b) in enumerate(self.layers):
            acc = np.broadcast_to(b, (x.shape[0], W.shape[0])).astype(self.dt)
            for k in range(W.shape[1]):  # k ascending, from the bias: policy_neuron's chain
                acc = _fma(x[:, k:k + 1], W[None, :, k], acc, self.f32)
            if l + 1 < len(self.layers):
                acc = np.tanh(acc.astype(F64)).astype(self.dt) if self.activation == "tanh" else np.maximum(acc, 0).astype(self.dt)
            x = acc
            xs.append(x)
        return xs

    def gradients(self, obs, target):
        """(loss, [(dW, db)]) of the batch (obs [B, 85], target [B, A])."""
        dt, f32 = self.dt, self.f32
        xs = self.forward(obs)
        B, A = target.shape
        e = xs[-1] - target.astype(dt)
        if f32:
            inv = F32(1) / F32(B * A)
            sq = F32(0)
            for v in e.ravel():  # (s, a) order, one fused chain
                sq = _fma(v, v, sq, True)
            loss, dscale = F32(sq * inv), F32(2) * inv
        else:
            loss, dscale = np.mean(e * e), 2.0 / (B * A)
        d = (dscale * e).astype(dt)
        grads = [None] * len(self.layers)
        for l in range(len(self.layers) - 1, -1, -1):
            x = xs[l]
            dW, db = np.zeros_like(self.layers[l][0]), np.zeros_like(self.layers[l][1])
            for s in range(B):  # the batch in index order
                dW = _fma(d[s][:, None], x[s][None, :], dW, f32)
                db = _fma(1.0, d[s], db, f32)
            grads[l] = (dW.astype(dt), db.astype(dt))
            if l:
                W = self.layers[l][0]
                back = np.zeros((B, W.shape[1]), dt)
                for j in range(W.shape[0]):  # j ascending from 0
                    back = _fma(d[:, j:j + 1], W[j][None, :], back, f32)
                a = xs[l]
                grad = _fma(-a, a, 1.0, f32) if self.activation == "tanh" else (a > 0).astype(dt)
                d = (back.astype(dt) * grad.astype(dt)).astype(dt)
        return loss, grads

    def step(self, obs, target, optimizer="sgd", lr=1.0, betas=(0.9, 0.999), eps=1e-8):
        """One optimisation step on the batch; returns the loss before it.  lr, betas and eps are taken at their
        fp32 values in both arithmetics (the device gets them as floats)."""
        loss, grads = self.gradients(obs, target)
        self.t += 1
        lr, eps, b1, b2 = (F32(v) for v in (lr, eps, betas[0], betas[1]))
        for l, (g, (W, b)) in enumerate(zip(grads, self.layers)):
            new = []
            for i in range(2):
                w = (W, b)[i]
                if optimizer == "sgd":
                    w = sgd32(w, g[i], lr) if self.f32 else w - F64(lr) * g[i]
                elif self.f32:
                    w, m, v = adam32(w, g[i], self.m[l][i], self.v[l][i], self.t, lr, b1, b2, eps)
                    self.m[l], self.v[l] = _set(self.m[l], i, m), _set(self.v[l], i, v)
                else:
                    w, m, v = adam64(w, g[i], self.m[l][i], self.v[l][i], self.t, F64(lr), F64(b1), F64(b2), F64(eps))
                    self.m[l], self.v[l] = _set(self.m[l], i, m), _set(self.v[l], i, v)
                new.append(w)
            self.layers[l] = tuple(new)
        return loss


def _set(pair, i, v):
    return (v, pair[1]) if i == 0 else (pair[0], v)


def sgd32(w, g, lr):
    return _fma(-F32(lr), g, w, True)


def adam64(w, g, m, v, t, lr, b1, b2, eps):
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    return w - lr * (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps), m, v


def adam32(w, g, m, v, t, lr, b1, b2, eps):
    """csrc/mmx_policy_fit.h's operation order on float32 arrays, one rounding per line."""
    w, g, m, v = (np.asarray(a, F32) for a in (w, g, m, v))
    lr, b1, b2, eps = F32(lr), F32(b1), F32(b2), F32(eps)
    omb1, omb2 = F32(1) - b1, F32(1) - b2
    c1 = F32(1.0 / (1.0 - F64(b1) ** t))
    c2 = F32(1.0 / (1.0 - F64(b2) ** t))
    t1 = omb1 * g
    m = _fma(b1, m, t1, True)
    t3 = (omb2 * g) * g
    v = _fma(b2, v, t3, True)
    mhat, vhat = m * c1, v * c2
    den = np.sqrt(vhat) + eps
    return w - (lr * mhat) / den, m, v


def fit(spec, obs, target, steps, batch, f32, optimizer="adam", shuffle=True, seed=0, k0=0, net=None, **opt):
    """`steps` optimisation steps from step counter k0; returns (losses, net)."""
    net = Net(spec, f32) if net is None else net
    net.t = k0
    losses = []
    for k in range(k0, k0 + steps):
        idx = batch_indices(shuffle, seed, k, batch, len(obs))
        losses.append(net.step(obs[idx], target[idx], optimizer, **opt))
    return np.array(losses), net


# ------------------------------------------------------------------ the shared cases
GRAD_CASES = [  # hidden, A, activation, bias
    ((), 4, "tanh", True), ((63,), 10, "relu", False), ((65, 64), 4, "tanh", True), ((256, 1, 255), 10, "relu", True),
    ((), 10, "relu", False), ((63,), 4, "tanh", True), ((65, 64), 10, "relu", False), ((256, 1, 255), 4, "tanh", False),
]


def make_case(hidden, A, activation, bias, n, seed=5):
    """A seeded policy and n pairs: observation entry 17 is huge and its scale 0 (the first layer's weights of that
    input get a gradient of exactly 0); the targets are an offset of a random teacher's outputs."""
    spec = make_spec(A, hidden=hidden, activation=activation, bias=bias, seed=seed + len(hidden) + A)
    spec["obs_scale"][17] = 0.0
    rng = np.random.default_rng(seed)
    obs = rng.uniform(-2.0, 2.0, (n, 85)).astype(F32)
    obs[:, 17] = F32(3e30)
    teacher = make_spec(A, hidden=(32,), activation="tanh", seed=seed + 100)
    teacher["obs_scale"][17] = 0.0
    target = (Net(teacher, False).forward(obs)[-1] + 0.3 * rng.standard_normal((n, A))).astype(F32)
    return spec, obs, target
