"""fp64 restatement of the MLP policy's forward pass (include/mmx_api.h, "Closed-loop MLP policies") with its
running forward-error bound, and the seeded policies of the tests: for tests/test_policy_host.py (CPU) and
tests/test_policy_rollout.py (GPU).

The bound, with u = 2^-24: a layer of n inputs adds 2 (n + 2) u (|W| |x| + |b|) (the fused accumulation's n + 1
roundings; the factor 2 covers fused against unfused products and the two roundings of the normalised input) to
|W| times the incoming error; a tanh unit adds ACT_EPS = 8 u (exp2 and reciprocal within one ulp each, and the
rounding of the exponent's argument, which the form 1 - 2 / (1 + e^2x) damps by |x| e^2x / (1 + e^2x)^2 < 0.5);
tanh and ReLU are 1-Lipschitz."""
import numpy as np

U = 2.0 ** -24
ACT_EPS = 8 * U
POLICY_SEED = 2024


def make_spec(A, hidden=(256, 256), activation="tanh", low=None, high=None, bias=True, seed=POLICY_SEED, log_std=None, spread=0.72,
              obs_gain=1.0):
    """Seeded random weights: hidden layers N(0, 1 / in); the last layer is centred on the box (or on 0) with a
    spread of `spread` half-widths per unit of hidden activity; obs_gain scales the observation's normalisation
    (how strongly the output follows the observation)."""
    rng = np.random.default_rng(seed)
    low = np.full(A, -1.0, np.float32) if low is None else low
    high = np.full(A, 1.0, np.float32) if high is None else high
    centre, half = (low.astype(np.float64) + high) / 2, (high.astype(np.float64) - low) / 2
    layers, n_in = [], 85
    for w in hidden:
        layers.append(((rng.standard_normal((w, n_in)) / np.sqrt(n_in)).astype(np.float32),
                       (0.1 * rng.standard_normal(w)).astype(np.float32) if bias else None))
        n_in = w
    W = rng.standard_normal((A, n_in)) / np.sqrt(n_in) * spread * half[:, None]
    layers.append((W.astype(np.float32), centre.astype(np.float32) if bias else None))
    return dict(layers=layers, activation=activation, obs_shift=(0.1 * rng.standard_normal(85)).astype(np.float32),
                obs_scale=(obs_gain * rng.uniform(0.5, 2.0, 85)).astype(np.float32), low=low, high=high, seed=77, log_std=log_std)


def forward64(spec, obs):
    """(mean, bound) in fp64 of the network on obs [n, 85] (float32 values)."""
    x = (obs.astype(np.float64) - spec["obs_shift"].astype(np.float64)) * spec["obs_scale"].astype(np.float64)
    err = np.zeros_like(x)
    L = len(spec["layers"])
    for k, (W, b) in enumerate(spec["layers"]):
        W64 = W.astype(np.float64)
        b64 = np.zeros(W.shape[0]) if b is None else b.astype(np.float64)
        n = W.shape[1]
        err = err @ np.abs(W64).T + 2 * (n + 2) * U * (np.abs(x) @ np.abs(W64).T + np.abs(b64))
        x = x @ W64.T + b64
        if k + 1 < L:
            if spec["activation"] == "tanh":
                x, err = np.tanh(x), err + ACT_EPS
            else:
                x = np.maximum(x, 0.0)
    return x, err
