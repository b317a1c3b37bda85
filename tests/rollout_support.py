"""What the rollout and snapshot tests share (a plain module, imported like policy_ref.py): seeded envs and
action rows, host copies of every sim-owned buffer, and the exact comparisons.  Seeds, env counts, action
widths and the row layout are arguments: each test module passes its own."""
import hashlib

import numpy as np

REL = "ee_pos_rot6d_g_rel"


def _buffers():
    from mujoco_manip_amd import _lib as L

    return {"qpos": (L.NQ, "<f4"), "qvel": (L.NV, "<f4"), "ctrl": (L.NU, "<f4"), "qacc_warmstart": (L.NV, "<f4"),
            "obs": (L.NOBS, "<f4"), "reward": (1, "<f4"), "done": (3, "<i4"), "reward_components": (6, "<f4"),
            "episode_i": (L.EPI_N, "<i4"), "episode_f": (L.EPF_N, "<f4"), "kin": (L.KIN_N, "<f4"), "target": (4, "<f4"),
            "contacts": (L.MAXCON * L.CON_F, "<f4")}


def snapshot(env) -> dict:
    """Host copies of every sim-owned buffer (and the camera images, if any), after the queued work."""
    import torch

    env.synchronize()
    torch.cuda.synchronize()
    out = {k: env.sim.view(k, w, t).cpu().numpy().copy() for k, (w, t) in _buffers().items()}
    if env._images is not None:
        out["images"], out["seg"] = env._images.cpu().numpy().copy(), env._seg.cpu().numpy().copy()
    return out


def make_env(n, mode="abs_pos", rows=None, image_size=0, *, seed, max_episode_steps=4, render_effects=(), lib=None):
    """n staged-reward envs with random spawns and autoreset, reset from `seed`; rows: the step kernel's row
    layout (None: the sim's own choice)."""
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(n, tasks="all", action_mode=mode, reward_type="staged", randomize_objects=True,
                          max_episode_steps=max_episode_steps, autoreset=True, image_size=image_size,
                          render_effects=render_effects, lib=lib)
    if rows is not None:
        env.sim.step_rows = rows
        assert env.sim.step_rows == rows
    env.reset(seed=seed)
    return env


def make_actions(mode: str, T: int, n: int, *, seed, widths) -> np.ndarray:
    """Seeded random targets inside the workspace, [T, n, widths[mode]]: a different one per env and step."""
    rng = np.random.default_rng(seed)
    a = np.zeros((T, n, widths[mode]), np.float32)
    grip = rng.integers(0, 2, (T, n)).astype(np.float32)
    if mode == "abs_pos":
        a[..., :3] = rng.uniform([-0.2, 0.3, 0.3], [0.2, 0.5, 0.5], (T, n, 3))
        a[..., 3] = grip
    else:  # a small offset from the initial EE pose, near-identity 6D rotation; columns from 10 on are not read
        a[..., :3] = rng.uniform(-0.1, 0.1, (T, n, 3))
        a[..., 3:9] = np.array([1, 0, 0, 0, 1, 0], np.float32) + rng.uniform(-0.05, 0.05, (T, n, 6))
        a[..., 9] = grip
        if widths[mode] > 10:
            a[..., 10:] = rng.uniform(-1e3, 1e3, (T, n, widths[mode] - 10))
    return a


def record_names():
    from mujoco_manip_amd import _lib

    return tuple(_lib.TRAJ_FIELDS)


def to_host(rec: dict) -> dict:
    import torch

    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in rec.items()}


def assert_record(rec: dict, snaps: list, skip=()):
    assert set(rec) == set(record_names())
    for name in record_names():
        if name in skip:
            continue
        want = np.stack([s[name] for s in snaps])
        assert rec[name].shape == want.shape and rec[name].dtype == want.dtype, name
        bad = np.argwhere(rec[name] != want)
        assert bad.size == 0, f"record '{name}' differs first at (step, env, ...) = {bad[0].tolist()}"


def assert_final(got: dict, want: dict):
    assert set(got) == set(want)
    for name in want:
        bad = np.argwhere(got[name] != want[name])
        assert bad.size == 0, f"buffer '{name}' differs first at {bad[0].tolist()}"


def digest(rec: dict) -> str:
    h = hashlib.sha256()
    for name in record_names():
        h.update(np.ascontiguousarray(rec[name]).tobytes())
    return h.hexdigest()


def bits(a: np.ndarray) -> np.ndarray:
    """The array's bytes as unsigned integers of its item size (a NaN equals itself, -0.0 differs from 0.0)."""
    return np.ascontiguousarray(a).view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def assert_same(got: dict, want: dict, skip=(), envs=None, axis=0, what=""):
    """Every array of `want` equals `got`'s, bit for bit; envs: only these indices along `axis`."""
    assert set(got) == set(want)
    for name in want:
        if name in skip:
            continue
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, name
        if envs is not None:
            g, w = np.take(g, envs, axis=axis), np.take(w, envs, axis=axis)
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, f"{what} '{name}' differs first at {bad[0].tolist()} ({len(bad)} words)"
