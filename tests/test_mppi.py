"""MPPI planning on the device (mmx_mppi_plan; mujoco_manip_amd.planner.MppiPlanner) against the fp64
restatements of tests/mppi_ref.py and against the library's own restore + rollout.

Shapes: M = 2 controlled envs with different seeds and tasks (abs_pos, staged reward, randomised objects),
advanced three expert steps so that cubes and arm are off the keyframe; K = 8 candidates, H = 3 steps,
sigma = (0.05, 0.05, 0.05, 0.6).

Bounds.  noise and actions: 4 * 2^-24 per unit of magnitude (a handful of fp32 operations on values of at most
about 1).  reward and done: bit for bit what an independent planner-shaped env records under restore(snap,
src = i // K) and rollout(actions).  returns: H * 2^-23 * max|r|.  weights: 2e-5 absolute; nominal and
action_out: 2e-5 * (high - low) (the exponent's argument is below 50 in magnitude, asserted, so its fp32
rounding moves a weight by at most 3e-6 relative; then a 1-2 ulp exponential and K summands).  The library's
own noise: 1e-4 absolute against the fp64 Philox / Box-Muller restatement (|z| <= 5.8 times the roughly 1e-6
absolute error expected of the hardware sine and cosine)."""
import ctypes as C

import numpy as np
import pytest

import mppi_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

M, K, H, A = 2, 8, 3, 4
N = M * K
SIGMA = (0.05, 0.05, 0.05, 0.6)
SEEDS, TASKS = [7, 1234], [("obj_red", "bin_blue"), ("obj_blue", "bin_red")]
# (staged rewards are about 0.1 a step: at this temperature the returns spread over a dozen lambda)
TEMPERATURE, GAMMA, BETA = 0.005, 0.95, 0.5
NOISE_SEED = 2**40 + 17
CFG = dict(tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True)


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def make_env(image_size=0, max_episode_steps=500, steps=3, n=M):
    """The controlled env: different seeds and tasks, `steps` expert steps off the keyframe."""
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(n, image_size=image_size, max_episode_steps=max_episode_steps, autoreset=False, **CFG)
    env.reset(seed=SEEDS[:n], options={"task": TASKS[:n]})
    for _ in range(steps):
        env.step(env.expert_plan())
    return env


def state(env):
    """The env's snapshot bytes, whole records.  (Taken into a zeroed tensor: env.snapshot() allocates an
    uninitialised one and the kernel writes the packed fields only, so the 12 bytes of padding behind them
    would be whatever the allocator left.)"""
    data = torch.zeros((env.num_envs, env.sim.snapshot_bytes), dtype=torch.uint8, device=env.device)
    env.sim.snapshot(data.data_ptr())
    return data


def make_planner(env, samples=K, horizon=H, temperature=TEMPERATURE, discount=GAMMA, noise_beta=BETA, seed=0):
    from mujoco_manip_amd.planner import MppiPlanner

    return MppiPlanner(env, samples, horizon, SIGMA, temperature=temperature, discount=discount, noise_beta=noise_beta,
                       seed=seed)


def run_plan(planner, a0, xi, snap=None):
    """reset(a0) + plan(xi): host copies of the nominal before the call, the output and every buffer after it."""
    planner.reset(a0)
    nominal0 = planner.buffers["nominal"].clone()
    out = planner.plan(xi=xi, snapshot=snap).clone()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy().copy() for k, v in planner.buffers.items()}
    got["nominal0"], got["action_out"] = nominal0.cpu().numpy(), out.cpu().numpy()
    return got


@pytest.fixture(scope="module")
def ctx():
    """The controlled env, its snapshot, the reset action, the caller's xi, and one planner per temperature."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    env = make_env()
    c = {"env": env, "snap": env.snapshot(), "a0": env.expert_plan(), "results": {}, "planners": {}}
    gen = torch.Generator(device=env.device).manual_seed(5)
    c["xi"] = torch.randn(H, N, A, generator=gen, device=env.device)
    yield c
    for p in c["planners"].values():
        p.close()
    env.close()


def planner_of(ctx, temperature):
    if temperature not in ctx["planners"]:
        ctx["planners"][temperature] = make_planner(ctx["env"], temperature=temperature)
    return ctx["planners"][temperature]


def result_of(ctx, temperature):
    """The composition test's call (caller-supplied xi, beta = 0.5), once per temperature."""
    if temperature not in ctx["results"]:
        ctx["results"][temperature] = run_plan(planner_of(ctx, temperature), ctx["a0"], ctx["xi"], ctx["snap"])
    return ctx["results"][temperature]


def box():
    from mujoco_manip_amd.planner import action_box

    low, high = action_box("abs_pos")
    return np.array(low), np.array(high)


def check_composition(got, xi, snap, a0, cfg, m, k, h, beta, sigma, low, high, temperature, gamma):
    """One plan call's buffers against the restatement and against an independent env's restore + rollout."""
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    n, low, high = m * k, np.asarray(low, np.float64), np.asarray(high, np.float64)
    # sample: filter, sigma, clamp
    noise, actions = mppi_ref.candidates(xi.cpu().numpy(), got["nominal0"], k, beta, sigma, low, high)
    for name, want in (("noise", noise), ("actions", actions)):
        err = np.abs(got[name] - want) / np.maximum(1.0, np.abs(want))
        print(name, "max error per unit of magnitude", err.max(), "bound", 4 * 2.0 ** -24)
        assert err.max() <= 4 * 2.0 ** -24
    assert (bits(got["actions"][:, ::k]) == bits(got["nominal0"])).all(), "candidate 0 is the nominal plan itself"
    assert (got["noise"][:, ::k] == 0).all() and (got["noise"][:, 1::k][..., np.asarray(sigma) > 0] != 0).all()
    assert (got["nominal0"] == np.clip(a0.cpu().numpy(), low.astype(np.float32), high.astype(np.float32))[None]).all()
    # branch + roll out: an independent planner-shaped env under restore(snap, src = i // K) and rollout(actions)
    ref = PickPlaceVecEnv(n, image_size=0, autoreset=False, **cfg)
    ref.reset(seed=99)
    ref.restore(snap, src=torch.arange(n, device=ref.device, dtype=torch.int32) // k)
    rec = ref.rollout(torch.as_tensor(got["actions"], device=ref.device), record=("reward", "done"))
    torch.cuda.synchronize()
    reward, done = rec["reward"].cpu().numpy(), rec["done"].cpu().numpy()
    ref.close()
    assert (bits(got["reward"]) == bits(reward)).all() and (got["done"] == done).all()
    for g in range(m):
        assert np.unique(reward[:, g * k:(g + 1) * k], axis=1).shape[1] > 1, "the candidates' rewards differ"
    # reweight, in fp64 on that recorded reward
    want = mppi_ref.update(reward, done, got["actions"], got["nominal0"], k, temperature, gamma)
    rmax = np.abs(reward).max()
    err = np.abs(got["returns"] - want["returns"]).max()
    print("returns: max error", err, "bound", h * 2.0 ** -23 * rmax, "max |r|", rmax)
    assert err <= h * 2.0 ** -23 * rmax
    assert (got["best"] == want["best"]).all()
    if temperature > 0:  # the premise of the 2e-5
        spread = (want["returns"].reshape(m, k).max(axis=1, keepdims=True) - want["returns"].reshape(m, k)) / temperature
        print("largest exponent argument", spread.max())
        assert spread.max() < 50
    else:
        onehot = np.zeros((m, k), np.float32)
        onehot[np.arange(m), want["best"]] = 1
        assert (got["weights"].reshape(m, k) == onehot).all()
    werr = np.abs(got["weights"] - want["weights"]).max()
    nerr = (np.abs(got["nominal"] - want["nominal"]) / (high - low)).max()
    oerr = (np.abs(got["action_out"] - want["action_out"]) / (high - low)).max()
    print("weights: max error", werr, "nominal, action_out: max error / (high - low)", nerr, oerr)
    assert werr <= 2e-5 and nerr <= 2e-5 and oerr <= 2e-5
    assert np.abs(got["weights"].reshape(m, k).sum(axis=1, dtype=np.float64) - 1).max() <= 2e-5
    assert (bits(got["nominal"][h - 1]) == bits(got["nominal"][h - 2])).all(), "the shift repeats the last step"


@pytest.mark.parametrize("temperature", (TEMPERATURE, 0.0))
def test_composition(ctx, temperature):
    low, high = box()
    check_composition(result_of(ctx, temperature), ctx["xi"], ctx["snap"], ctx["a0"], CFG, M, K, H, BETA, SIGMA, low, high,
                      temperature, GAMMA)


REL = "ee_pos_rot6d_g_rel"
# the update kernel's other paths: a partly filled second wave (K = 65), more candidates than its 256 lanes
# (K = 300: two per lane; the sums stay lane-strided partials and a tree, far inside the 2e-5 derived for 256
# summands in a row), and ten action components (a row that is no power of two, the widest accumulator set)
OTHER_SHAPES = {"K65": ("abs_pos", 1, 65), "K300": ("abs_pos", 1, 300), "A10": (REL, 2, 8)}


@pytest.mark.parametrize("shape", sorted(OTHER_SHAPES))
def test_composition_other_shapes(shape):
    from mujoco_manip_amd.planner import MppiPlanner
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    mode, m, k = OTHER_SHAPES[shape]
    h, cfg = 2, dict(CFG, action_mode=mode)
    env = PickPlaceVecEnv(m, image_size=0, autoreset=False, **cfg)
    env.reset(seed=SEEDS[:m], options={"task": TASKS[:m]})
    if mode == "abs_pos":
        low, high = box()
        sigma, a0 = SIGMA, env.expert_plan()
    else:  # an offset from the initial EE pose, a 6D rotation near the identity, the gripper
        low = np.array([-0.3] * 3 + [-1.5] * 6 + [0.0])
        high = np.array([0.3] * 3 + [1.5] * 6 + [1.0])
        sigma = (0.05,) * 3 + (0.02,) * 6 + (0.6,)
        a0 = torch.tensor([[0.02, -0.03, -0.05, 1, 0, 0, 0, 1, 0, 1.0]] * m, device=env.device)
    for _ in range(2):
        env.step(a0)
    p = MppiPlanner(env, k, h, sigma, temperature=TEMPERATURE, discount=GAMMA, noise_beta=BETA, seed=0, low=low, high=high)
    try:
        snap = env.snapshot()
        gen = torch.Generator(device=env.device).manual_seed(k)
        xi = torch.randn(h, m * k, env.action_dim, generator=gen, device=env.device)
        got = run_plan(p, a0, xi, snap)
        check_composition(got, xi, snap, a0, cfg, m, k, h, BETA, sigma, low, high, TEMPERATURE, GAMMA)
    finally:
        p.close()
        env.close()


def test_library_noise(ctx):
    env, a0, snap = ctx["env"], ctx["a0"], ctx["snap"]
    p1, p2 = (make_planner(env, noise_beta=0.0, seed=NOISE_SEED) for _ in range(2))
    p4 = make_planner(env, samples=4, noise_beta=0.0, seed=NOISE_SEED)
    try:
        g1, g2, g4 = (run_plan(p, a0, None, snap) for p in (p1, p2, p4))
        for call, got in ((0, g1), (1, None)):
            if got is None:  # a second call: call index 1
                out = p1.plan(snapshot=snap).clone()
                torch.cuda.synchronize()
                got = {"noise": p1.buffers["noise"].cpu().numpy().copy()}
                assert (bits(got["noise"]) != bits(g1["noise"])).any()
                assert (bits(got["noise"][:, 1]) != bits(g1["noise"][:, 1])).all(), "every element is drawn anew"
                del out
                noise1 = got["noise"]
            want = mppi_ref.draw_array(NOISE_SEED, call, H, N, A)
            want[:, ::K] = 0.0
            err = np.abs(got["noise"] - want).max()
            print("library noise, call", call, ": max |device - fp64| =", err, "largest |z|", np.abs(want).max())
            assert err <= 1e-4
        for name in ("noise", "actions", "weights", "action_out"):
            assert (bits(g1[name]) == bits(g2[name])).all(), f"two planners with one seed differ in '{name}'"
        # the counter counts calls with the caller's xi too, and reset puts it back to 0
        p2.reset(a0)
        p2.plan(xi=ctx["xi"], snapshot=snap)
        p2.plan(snapshot=snap)
        torch.cuda.synchronize()
        assert (bits(p2.buffers["noise"].cpu().numpy()) == bits(noise1)).all(), "xi call, then the library's call 1"
        p2.reset(a0)
        p2.plan(snapshot=snap)
        torch.cuda.synchronize()
        assert (bits(p2.buffers["noise"].cpu().numpy()) == bits(g1["noise"])).all(), "after reset: call 0 again"
        # the draw depends on (seed, call, t, i, a) alone: K = 4 on M * 4 envs draws what K = 8 draws for i < 8
        rows = [i for i in range(M * 4) if i % 4 and i % K]
        assert len(rows) == 6
        assert (bits(g4["noise"][:, rows]) == bits(g1["noise"][:, rows])).all()
        assert (g4["noise"][:, ::4] == 0).all()
    finally:
        for p in (p1, p2, p4):
            p.close()


def test_episode_end_inside_the_horizon():
    """max_episode_steps = 2 in both sims, a fresh controlled env, H = 4: every candidate is truncated at t = 1."""
    env = make_env(max_episode_steps=2, steps=0)
    p = make_planner(env, horizon=4, discount=0.9, noise_beta=0.0, seed=3)
    try:
        assert int(p.sim_env.sim.cfg.max_episode_steps) == 2
        got = run_plan(p, env.expert_plan(), None)
        assert (got["done"][0, :, 1] == 0).all() and (got["done"][1, :, 1] == 1).all()
        r = got["reward"].astype(np.float64)
        want = r[0] + 0.9 * r[1]
        err = np.abs(got["returns"] - want).max()
        print("returns: max error", err, "bound", 4 * 2.0 ** -23 * np.abs(r).max())
        assert err <= 4 * 2.0 ** -23 * np.abs(r).max()
        R0, _ = mppi_ref.returns(got["reward"], got["done"], 0.9)
        changed = got["reward"].copy()
        changed[2:] = changed[2:] * -3.0 + 7.0
        R1, alive = mppi_ref.returns(changed, got["done"], 0.9)
        assert (R0 == R1).all() and (R0 == want).all() and not alive[2:].any() and alive[:2].all()
    finally:
        p.close()
        env.close()


@pytest.mark.parametrize("temperature", (TEMPERATURE, 0.0))
def test_non_finite_returns_are_excluded_on_the_device(ctx, temperature):
    """The reweight kernel alone (mmx_mppi_reweight) on the composition call's actions with planted rewards: in
    group 0 the best candidate's return becomes +Inf and another's NaN (both excluded: the +Inf must not win), a
    third candidate has a NaN reward behind its episode's end (it stays in); group 1 is excluded whole (weights
    0, best -1, nominal kept bit for bit, action_out = its first step).  Bounds as in the composition test."""
    p = planner_of(ctx, temperature)
    base = run_plan(p, ctx["a0"], ctx["xi"], ctx["snap"])
    p.reset(ctx["a0"])  # the nominal as before that call
    reward, done = base["reward"].copy(), base["done"].copy()
    assert not done[:, :, :2].any()
    k_inf = int(base["best"][0])
    k_nan, k_end = (k_inf + 1) % K, (k_inf + 2) % K
    reward[0, k_inf], reward[1, k_nan] = np.inf, np.nan
    done[0, k_end, 0], reward[1, k_end] = 1, np.nan
    reward[H - 1, K:] = np.where(np.arange(K) % 2, np.nan, -np.inf)
    p.buffers["reward"].copy_(torch.as_tensor(reward))
    p.buffers["done"].copy_(torch.as_tensor(done))
    out = torch.zeros(M, A, device=ctx["env"].device)
    p.mppi.reweight(out.data_ptr())
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in p.buffers.items()}
    want = mppi_ref.update(reward, done, base["actions"], base["nominal0"], K, temperature, GAMMA)
    fin = np.isfinite(want["returns"])
    assert fin.sum() == K - 2 and fin[k_end] and not fin[k_inf] and not fin[k_nan] and not fin[K:].any()
    assert (np.isfinite(got["returns"]) == fin).all()
    assert np.abs(got["returns"][fin] - want["returns"][fin]).max() <= H * 2.0 ** -23 * np.abs(base["reward"]).max()
    assert (got["best"] == want["best"]).all() and got["best"][1] == -1 and got["best"][0] not in (k_inf, k_nan)
    assert (got["weights"][~fin] == 0).all() and np.isfinite(got["weights"]).all()
    assert np.abs(got["weights"] - want["weights"]).max() <= 2e-5
    assert abs(got["weights"][:K].sum(dtype=np.float64) - 1) <= 2e-5
    low, high = box()
    assert np.isfinite(got["nominal"]).all()
    assert (np.abs(got["nominal"] - want["nominal"]) / (high - low)).max() <= 2e-5
    assert (np.abs(out.cpu().numpy() - want["action_out"]) / (high - low)).max() <= 2e-5
    assert (bits(got["nominal"][:, 1]) == bits(base["nominal0"][:, 1])).all(), "the excluded group's nominal is kept"
    assert (bits(out.cpu().numpy()[1]) == bits(base["nominal0"][0, 1])).all()
    # the planner goes on as before
    again = run_plan(p, ctx["a0"], ctx["xi"], ctx["snap"])
    assert (bits(again["action_out"]) == bits(base["action_out"])).all()


def test_state_from_an_env_with_cameras(ctx):
    """The same seed and steps with image_size = 16: 1,920-byte records, the same plan bit for bit."""
    from mujoco_manip_amd import _lib

    cam = make_env(image_size=16)
    try:
        snap = cam.snapshot()
        assert snap.rec_bytes == 1920 and ctx["snap"].rec_bytes == 1248
        p = planner_of(ctx, TEMPERATURE)
        want = result_of(ctx, TEMPERATURE)
        got = run_plan(p, ctx["a0"], ctx["xi"], snap)
        for name in ("action_out", "reward", "done", "returns", "weights", "nominal"):
            assert (bits(got[name]) == bits(want[name])).all(), name
        # mmx_restore itself keeps rejecting the size mismatch
        sim = p.sim_env.sim
        assert sim.L.mmx_restore(sim.ptr, C.c_void_p(snap.data.data_ptr()), 1920, M, None) == -1
        assert sim.L.mmx_restore(sim.ptr, C.c_void_p(ctx["snap"].data.data_ptr()), 1248, M, None) == 0
        torch.cuda.synchronize()
        assert _lib.snapshot_record_bytes(True) == 1920
    finally:
        cam.close()


def test_controlled_sim_is_untouched():
    env, twin = make_env(), make_env()
    p = make_planner(env, noise_beta=0.0, seed=11)
    try:
        p.reset(env.expert_plan())
        before = state(env)
        p.plan()
        assert torch.equal(before, state(env))
        assert torch.equal(before, state(twin))
        log = []
        for _ in range(10):  # closed loop: the planner plans from, and never writes to, the env it controls
            a = p.plan().clone()
            log.append(a)
            env.step(a)
        for a in log:
            twin.step(a)
        assert len({bytes(bits(a.cpu().numpy())) for a in log}) > 1
        assert not torch.equal(before, state(env))
        assert torch.equal(state(env), state(twin))
    finally:
        p.close()
        env.close()
        twin.close()


def test_arguments(ctx):
    from mujoco_manip_amd import _lib

    p = planner_of(ctx, TEMPERATURE)
    want = result_of(ctx, TEMPERATURE)
    sim, L = p.sim_env.sim, p.sim_env.sim.L
    snap, xi = ctx["snap"], ctx["xi"].contiguous()
    blob, out = snap.data.data_ptr(), torch.zeros(M, A, device=ctx["env"].device)
    assert blob % 16 == 0
    vp = C.c_void_p
    bad = {"NULL planner": (None, vp(blob), 1248, M, vp(xi.data_ptr()), vp(out.data_ptr())),
           "NULL blob": (p.mppi.ptr, None, 1248, M, vp(xi.data_ptr()), vp(out.data_ptr())),
           "NULL output": (p.mppi.ptr, vp(blob), 1248, M, vp(xi.data_ptr()), None),
           "unaligned blob": (p.mppi.ptr, vp(blob + 4), 1248, M, vp(xi.data_ptr()), vp(out.data_ptr())),
           "rec_bytes 1264": (p.mppi.ptr, vp(blob), 1264, M, vp(xi.data_ptr()), vp(out.data_ptr())),
           "rec_bytes 0": (p.mppi.ptr, vp(blob), 0, M, vp(xi.data_ptr()), vp(out.data_ptr())),
           "n_records M - 1": (p.mppi.ptr, vp(blob), 1248, M - 1, vp(xi.data_ptr()), vp(out.data_ptr())),
           "n_records M + 1": (p.mppi.ptr, vp(blob), 1248, M + 1, vp(xi.data_ptr()), vp(out.data_ptr()))}
    for what, args in bad.items():
        assert L.mmx_mppi_plan(*args) == -1, what
        got = run_plan(p, ctx["a0"], ctx["xi"], snap)
        for name in ("action_out", "noise", "actions", "reward", "done", "returns", "weights", "best", "nominal"):
            assert (bits(got[name]) == bits(want[name])).all(), (what, name)
    torch.cuda.synchronize()
    assert not out.any(), "a refused call launches nothing"

    def config(**kw):
        low, high = box()
        c = _lib.MMXMppiConfig(horizon=H, samples=K, temperature=TEMPERATURE, discount=GAMMA, noise_beta=BETA, seed=0)
        for a in range(A):
            c.sigma[a], c.low[a], c.high[a] = SIGMA[a], low[a], high[a]
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    def create(s, c):
        ptr = C.c_void_p()
        rc = L.mmx_mppi_create(s.ptr, C.byref(c), C.byref(ptr))
        if rc == 0:
            L.mmx_mppi_destroy(ptr)
        else:
            assert not ptr.value
        return rc

    assert create(sim, config()) == 0
    nan = float("nan")
    for kw in (dict(horizon=0), dict(horizon=65), dict(samples=1), dict(samples=5), dict(samples=N * 2), dict(temperature=-1.0),
               dict(temperature=nan), dict(temperature=1e-45), dict(temperature=float("inf")), dict(discount=0.0), dict(discount=1.5), dict(discount=nan), dict(noise_beta=-0.1),
               dict(noise_beta=1.0), dict(noise_beta=nan), dict(sigma=(1, -1.0)), dict(sigma=(3, nan)), dict(low=(2, 0.7)),
               dict(high=(0, -0.6))):
        assert create(sim, config(**kw)) == -1, kw
    assert create(sim, config(sigma=(A, -1.0), low=(A, 1.0), high=(A, 0.0))) == 0, "only the first A components are read"
    cam = make_env(image_size=16, steps=0)
    try:
        assert create(cam.sim, config(samples=2)) == -1, "a planner sim with cameras"
    finally:
        cam.close()
    got = run_plan(p, ctx["a0"], ctx["xi"], snap)
    assert (bits(got["action_out"]) == bits(want["action_out"])).all()
