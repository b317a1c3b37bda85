"""numpy / pure-Python fp64 restatements of the MPPI planner's closed forms (include/mmx_api.h, mmx_mppi_plan),
written from the header's text, for tests/test_mppi_host.py (CPU) and tests/test_mppi.py (GPU)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """The published algorithm (Salmon et al. 2011) on Python ints."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def draw(seed, call, t, i, a):
    """(u1, u2, z) of noise element (t, i, a) of call `call` under `seed`, in fp64."""
    x = philox4x32_10((call & MASK, call >> 32, i, 4 * t + a // 4), (seed & MASK, seed >> 32))
    xa, xb = (x[2], x[3]) if a % 4 >= 2 else (x[0], x[1])
    u1, u2 = ((xa >> 8) + 1) * 2.0 ** -24, (xb >> 8) * 2.0 ** -24
    r, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return u1, u2, float(r * (np.sin(ang) if a % 2 else np.cos(ang)))


def draw_array(seed, call, H, N, A):
    """xi [H, N, A] of the library's own draw."""
    return np.array([[[draw(seed, call, t, i, a)[2] for a in range(A)] for i in range(N)] for t in range(H)])


def candidates(xi, nominal, K, beta, sigma, low, high):
    """(noise, actions) [H, N, A] in fp64 from draws xi [H, N, A] and the nominal plans [H, M, A]."""
    xi = np.asarray(xi, np.float64)
    H, N, A = xi.shape
    eps = np.empty_like(xi)
    eps[0] = xi[0]
    for t in range(1, H):
        eps[t] = beta * eps[t - 1] + np.sqrt(1.0 - beta * beta) * xi[t]
    eps[:, ::K] = 0.0  # candidate 0 of every group is the nominal plan
    nom = np.repeat(np.asarray(nominal, np.float64), K, axis=1)
    return eps, np.clip(nom + np.asarray(sigma, np.float64) * eps, low, high)


def returns(reward, done, gamma):
    """R [N] in fp64 and the alive mask [H, N]: the ending step's reward counts, nothing after it."""
    reward = np.asarray(reward)
    H, N = reward.shape
    ended = (np.asarray(done)[:, :, 0] != 0) | (np.asarray(done)[:, :, 1] != 0)
    alive = np.ones((H, N), bool)
    for t in range(1, H):
        alive[t] = alive[t - 1] & ~ended[t - 1]
    g = gamma ** np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        R = np.where(alive, g * reward.astype(np.float64), 0.0).sum(axis=0)
    return R, alive


def update(reward, done, actions, nominal, K, temperature, gamma):
    """The reweighting in fp64 -> dict(returns, weights, best, nominal (shifted), action_out)."""
    R, _ = returns(reward, done, gamma)
    actions = np.asarray(actions, np.float64)
    H, N, A = actions.shape
    M = N // K
    nominal = np.array(nominal, np.float64)
    w, best, out = np.zeros(N), np.full(M, -1), np.empty((M, A))
    for m in range(M):
        Rm, ok = R[m * K:(m + 1) * K], np.isfinite(R[m * K:(m + 1) * K])
        if not ok.any():
            out[m] = nominal[0, m]
            continue
        k = int(np.argmax(np.where(ok, Rm, -np.inf)))  # the first maximum: lowest k on ties
        best[m] = k
        if temperature > 0:
            e = np.where(ok, np.exp((np.where(ok, Rm, Rm[k]) - Rm[k]) / temperature), 0.0)
        else:
            e = np.zeros(K)
            e[k] = 1.0
        w[m * K:(m + 1) * K] = e / e.sum()
        new = np.einsum("k,tka->ta", w[m * K:(m + 1) * K], actions[:, m * K:(m + 1) * K])
        out[m] = new[0]
        nominal[:, m] = np.concatenate([new[1:], new[-1:]])
    return {"returns": R, "weights": w, "best": best, "nominal": nominal, "action_out": out}
