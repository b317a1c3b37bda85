"""MppiPlanner — MPPI control of every env of a PickPlaceVecEnv, on the device (mmx_mppi_plan, include/mmx_api.h).

The planner owns a camera-less PickPlaceVecEnv of ``env.num_envs * samples`` envs with the controlled env's
configuration and no autoreset, on the same device and stream.  Every ``plan()`` snapshots the controlled env
and makes one library call: sample ``samples`` candidate action sequences around each env's nominal plan,
start the candidates' envs from their env's record, roll them out for ``horizon`` steps, reweight, and return
the first action of every new nominal plan.  Nothing is read back to the host; the controlled env is never
touched (it may have cameras: the planner reads the camera-less prefix of its records).

    planner = MppiPlanner(env, samples=256, horizon=4, sigma=(0.05, 0.05, 0.05, 0.6), temperature=0.05)
    planner.reset(env.expert_plan())          # or any action [M, A]: every step of every nominal plan
    for _ in range(steps):
        env.step(planner.plan())
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from . import _lib
from .gym_env import make_action_space
from .vec_env import PickPlaceVecEnv

_F32_MAX = float(np.finfo(np.float32).max)


def action_box(action_mode: str):
    """(low, high) of the action mode's Box (gym_env.make_action_space), unbounded components at +-float32 max."""
    sp = make_action_space(action_mode)
    return (np.clip(sp.low.astype(np.float64), -_F32_MAX, _F32_MAX).tolist(),
            np.clip(sp.high.astype(np.float64), -_F32_MAX, _F32_MAX).tolist())


class MppiPlanner:
    def __init__(self, env: PickPlaceVecEnv, samples: int, horizon: int, sigma, temperature: float = 1.0,
                 discount: float = 1.0, noise_beta: float = 0.0, seed: int = 0, low=None, high=None):
        self.env = env
        self.M, self.K, self.H, self.A = env.num_envs, int(samples), int(horizon), env.action_dim
        box_low, box_high = action_box(env._action_mode)
        low = box_low if low is None else list(low)
        high = box_high if high is None else list(high)
        sigma = [float(sigma)] * self.A if np.isscalar(sigma) else list(sigma)
        if self.K < 2:
            raise ValueError(f"samples must be at least 2, got {samples}")
        c = env.sim.cfg
        with self._on_env_stream():  # the planner sim takes the current stream: the controlled env's
            self.sim_env = PickPlaceVecEnv(
                self.M * self.K, task=env._fixed_task, tasks=env._task_pool, action_mode=env._action_mode,
                reward_type=env._reward_type, image_size=0, max_episode_steps=int(c.max_episode_steps),
                randomize_objects=bool(c.randomize_objects), spawn_x_range=tuple(c.spawn_x_range),
                spawn_y_range=tuple(c.spawn_y_range), autoreset=False, device=int(c.device),
                solver_iterations=int(c.solver_iterations), solver_tolerance=float(c.solver_tolerance),
                lib=env.sim.L._name)  # the controlled env's build of the library
        try:
            self.mppi = _lib.Mppi(self.sim_env.sim, horizon=self.H, samples=self.K, sigma=sigma, low=low, high=high,
                                  temperature=temperature, discount=discount, noise_beta=noise_beta, seed=seed)
        except Exception:
            self.sim_env.close()
            raise
        self.sim_env.reset(seed=seed)  # a defined state before the first branch overwrites it
        self.buffers = self.mppi.views()
        self._action = torch.zeros(self.M, self.A, device=env.device, dtype=torch.float32)

    def _on_env_stream(self):
        s = self.env.sim.cfg.stream
        if not s:
            return contextlib.nullcontext()
        return torch.cuda.stream(torch.cuda.ExternalStream(s, device=self.env.device))

    def reset(self, action):
        """Every step of every nominal plan = action [M, A] (kept within [low, high]); the call counter to 0."""
        a = torch.as_tensor(action, dtype=torch.float32, device=self.env.device)
        if tuple(a.shape) != (self.M, self.A):
            raise ValueError(f"action must be [{self.M}, {self.A}], got {tuple(a.shape)}")
        self._reset_action = a.contiguous()
        self.mppi.reset(self._reset_action.data_ptr())

    def plan(self, xi=None, snapshot=None) -> torch.Tensor:
        """One control step -> action [M, A] (a planner-owned tensor, overwritten by the next call).  xi: None
        (the library's Philox draw) or standard-normal draws [H, M * K, A]; snapshot: a Snapshot of the
        controlled env taken by the caller (None: taken here)."""
        snap = self.env.snapshot() if snapshot is None else snapshot
        if snap.num_envs != self.M or snap.data.device != self.env.device:
            raise ValueError(f"the snapshot must hold the {self.M} controlled envs on {self.env.device}")
        x = None
        if xi is not None:
            x = torch.as_tensor(xi, dtype=torch.float32, device=self.env.device).contiguous()
            if tuple(x.shape) != (self.H, self.M * self.K, self.A):
                raise ValueError(f"xi must be [{self.H}, {self.M * self.K}, {self.A}], got {tuple(x.shape)}")
        self._last = (snap, x)  # alive until the stream has run the call
        self.mppi.plan(snap.data.data_ptr(), snap.rec_bytes, snap.num_envs, None if x is None else x.data_ptr(),
                       self._action.data_ptr())
        return self._action

    def close(self):
        self.mppi.close()
        self.sim_env.close()
