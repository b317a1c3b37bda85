"""Pure-Python restatement of the DAgger gate (include/mmx_api.h, "DAgger rollouts"), written from the header's
text on the Philox restatement of tests/mppi_ref.py: for tests/test_dagger_host.py (CPU) and
tests/test_dagger_rollout.py (GPU)."""
import numpy as np

import mppi_ref

MASK = 0xFFFFFFFF


def gate_uniform(seed, call, t, i):
    """u of (seed, call, t, i): Philox4x32-10 with key = seed, counter = (call low, call high, i, 4 t + 3); the second
    output word's top 24 bits, times 2^-24.  Exact in fp32 and fp64 alike."""
    x = mppi_ref.philox4x32_10((call & MASK, call >> 32, i, 4 * t + 3), (seed & MASK, seed >> 32))
    return (x[1] >> 8) * 2.0 ** -24


def uniform_array(seed, call, T, N):
    return np.array([[gate_uniform(seed, call, t, i) for i in range(N)] for t in range(T)])


def dist2_f32(p, e):
    """The takeover's squared distance with the device's roundings: fp32 differences, then fma(dz, dz, fma(dy, dy,
    dx dx)), every step rounded once (a product of two fp32 numbers and the fused sum are exact in fp64 before the
    rounding, up to a double rounding the caller's comparison allows for by taking the value as an estimate only)."""
    p, e = np.asarray(p, np.float32), np.asarray(e, np.float32)
    d = (p[..., :3] - e[..., :3]).astype(np.float64)
    xx = (d[..., 0] * d[..., 0]).astype(np.float32).astype(np.float64)
    yy = (d[..., 1] * d[..., 1] + xx).astype(np.float32).astype(np.float64)
    return (d[..., 2] * d[..., 2] + yy).astype(np.float32)
