"""PickPlaceVecEnv — batched torch façade over the C-ABI (one MI355X, num_envs lanes).

Mirrors PickPlaceGymEnv (mujoco_manip/gym_env.py:39-602) with a leading env dimension:
same constructor keywords, same 5 action modes, same numeric observation keys and reward
types.  Differences, all documented in DESIGN.md:
  * observations are torch tensors on the GPU ([N, ...]); with image_size > 0 the
    `image_overhead` / `image_wrist` keys are uint8 [N, S, S, 3] from the batched HIP rasteriser
    (mmx_render.hip: the Panda's visual parts reduced to convex pieces and clustered meshes per
    part, flat-lit with the scene's lights, no specular), image_size = 0 skips them.
    By default nothing casts a shadow and the bins are opaque; render_effects=("shadows",
    "translucent_bins") (either or both) turns on the directional light's cast shadows and the
    bins' alpha 0.4, as the reference's mujoco.Renderer draws them (segment ids are the same);
  * reset(seed=s) seeds env i with s + i (gymnasium vector convention); a list gives one
    seed per env;
  * with autoreset=True an env that terminated/truncated (or whose FSM expert finished: reported
    as truncated) is reset inside the same step (the returned obs is the first obs of the new
    episode);
  * lib=<path> runs the env on that build of the library (_lib.load: a test build, a library of another
    revision) beside envs on other builds; None is the process's default.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .constants import ACTION_REPEAT, BINS, IMAGE_SIZE, MAX_EPISODE_STEPS, OBJECTS, OBS_SLICES, TASK_SETS, task_index
from .dagger import DEFAULT_RECORD as DAGGER_RECORD, check_args as check_dagger_args


def split_obs(flat: torch.Tensor) -> dict:
    """The numeric observation keys of a flat observation [..., 85] (OBS_SLICES on the last axis), as views."""
    return {k: flat[..., a:b].reshape(*flat.shape[:-1], *shape) for k, (a, b, shape) in OBS_SLICES.items()}


def check_gae_args(reward, done, value, value_last, gamma, lam, device):
    """What PickPlaceVecEnv.gae asks of its arguments, before the library is touched."""
    device = torch.device(device)
    if not (isinstance(reward, torch.Tensor) and reward.dim() == 2 and reward.shape[1] >= 1):
        raise ValueError("reward must be a torch tensor [T, N] with N >= 1")
    T, N = reward.shape
    if T * N >= 2**31:
        raise ValueError(f"reward has {T * N} entries; gae takes at most 2^31 - 1")
    for name, t, shape, dtype in (("reward", reward, (T, N), torch.float32), ("done", done, (T, N, 3), torch.int32),
                                  ("value", value, (T, N), torch.float32), ("value_last", value_last, (N,), torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError(f"{name} must be a {dtype} torch tensor of shape {shape}")
        if t.device != device:
            raise ValueError(f"{name} must be on {device}, got {t.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if not (0.0 <= float(gamma) <= 1.0 and 0.0 <= float(lam) <= 1.0):  # (a NaN fails both)
        raise ValueError(f"gamma and lam must be in [0, 1], got {gamma} and {lam}")


class Snapshot:
    """The state of `num_envs` environments on the device (PickPlaceVecEnv.snapshot): `data` is the uint8
    tensor [num_envs, rec_bytes] of their records (include/mmx_api.h; _lib.snapshot_field_offsets gives
    the fields of a row).  It may be restored any number of times, into any env with the same record size
    (cameras or not) on the same device, whatever its num_envs."""

    def __init__(self, data: torch.Tensor):
        assert data.dtype == torch.uint8 and data.dim() == 2 and data.is_contiguous()
        self.data = data
        self.num_envs, self.rec_bytes = int(data.shape[0]), int(data.shape[1])

    def clone(self) -> "Snapshot":
        return Snapshot(self.data.clone())


class PickPlaceVecEnv:
    metadata = {"render_modes": [], "render_fps": 30}

    def __init__(self, num_envs: int = 1, task: tuple[str, str] | None = None, tasks="all",
                 action_mode: str = "ee_pos_quat_g_rel", reward_type: str = "dense", image_size: int = IMAGE_SIZE,
                 render_mode: str | None = None, max_episode_steps: int = MAX_EPISODE_STEPS,
                 randomize_objects: bool = False, spawn_x_range=(-0.20, 0.20), spawn_y_range=(0.30, 0.45),
                 autoreset: bool = False, device: int = 0, solver_iterations: int = 30,
                 solver_tolerance: float = 1e-6, render_effects=(), lib: str | None = None):
        if not torch.cuda.is_available():
            raise RuntimeError("PickPlaceVecEnv needs an MI355X GPU (HIP); no CPU fallback exists")
        pool = TASK_SETS[tasks] if isinstance(tasks, str) else list(tasks)
        self.num_envs = int(num_envs)
        self.device = torch.device(f"cuda:{device}")
        self.render_mode = render_mode
        self._action_mode = action_mode
        self._reward_type = reward_type
        self._task_pool = pool
        self._fixed_task = task
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
        self.sim = _lib.Sim(self.num_envs, action_mode=action_mode, reward_type=reward_type,
                            max_episode_steps=max_episode_steps, randomize_objects=randomize_objects,
                            spawn_x_range=spawn_x_range, spawn_y_range=spawn_y_range,
                            task_pool=[task_index(t) for t in pool],
                            fixed_task=None if task is None else task_index(task), image_size=image_size,
                            autoreset=autoreset, solver_iterations=solver_iterations,
                            solver_tolerance=solver_tolerance, device=device, stream=stream,
                            render_effects=render_effects, lib=lib)
        s = self.sim
        self.action_dim = s.action_dim
        self._obs = s.view("obs", _lib.NOBS)
        self._reward = s.view("reward", 1)
        self._done = s.view("done", 3, "<i4")
        self._rc = s.view("reward_components", 6)
        self._epi = s.view("episode_i", _lib.EPI_N, "<i4")
        self._epf = s.view("episode_f", _lib.EPF_N)
        self.qpos = s.view("qpos", _lib.NQ)
        self.qvel = s.view("qvel", _lib.NV)
        self.ctrl = s.view("ctrl", _lib.NU)
        self.stats = s.view("stats", _lib.STAT_N)
        self._expert_action = torch.zeros(self.num_envs, 4, device=self.device, dtype=torch.float32)
        iv = s.image_views()
        self._images, self._seg = iv if iv is not None else (None, None)

    # ------------------------------------------------------------------ gym API
    def _obs_dict(self):
        flat = self._obs
        out = {}
        for k, (a, b, shape) in OBS_SLICES.items():
            out[k] = flat[:, a:b].reshape(self.num_envs, *shape).clone()
        if self._images is not None:  # gym_env.py:325-326
            out["image_overhead"] = self._images[:, 0].clone()
            out["image_wrist"] = self._images[:, 1].clone()
        return out

    @property
    def segmentation(self) -> torch.Tensor | None:
        """Segment ids [N, 2, S, S] of the last rendered images (overhead, wrist), or None."""
        return None if self._seg is None else self._seg.clone()

    def reset(self, *, seed=None, options: dict | None = None):
        """PickPlaceGymEnv.reset (gym_env.py:477-534), batched."""
        N = self.num_envs
        seeds = None
        if seed is not None:
            seeds = [int(seed) + k for k in range(N)] if np.isscalar(seed) else list(seed)
        task = None
        if options and "task" in options:
            t = options["task"]
            if isinstance(t, tuple) and isinstance(t[0], str):
                o, b = task_index(t)
                task = np.full(N, (o << 4) | b, np.int32)
            else:
                task = np.array([(task_index(x)[0] << 4) | task_index(x)[1] for x in t], np.int32)
        self.sim.reset(seeds=seeds, task_override=task)
        return self._obs_dict(), {}

    def synchronize(self):
        """Wait for the env's queued launches.  Raises the reference's RuntimeError (randomization.py:84-87)
        when an autoreset since the last reset / synchronize exhausted its spawn sampling (that env's
        env_error carries bit 8 and its cubes stay at the keyframe, as where the reference raises)."""
        self.sim.synchronize()

    def step(self, actions: torch.Tensor):
        """PickPlaceGymEnv.step (gym_env.py:536-581), batched: actions [N, action_dim] fp32 on the GPU."""
        a = torch.as_tensor(actions, dtype=torch.float32, device=self.device)
        if a.dim() != 2 or a.shape[0] != self.num_envs or a.shape[1] < self.action_dim:
            raise ValueError(f"actions must be [{self.num_envs}, {self.action_dim}], got {tuple(a.shape)}")
        a = a.contiguous()
        self.sim.step(a.data_ptr(), a.shape[1])
        obs = self._obs_dict()
        reward = self._reward.clone()
        terminated = self._done[:, 0].bool().clone()
        truncated = self._done[:, 1].bool().clone()
        info = {"success": self._done[:, 2].bool().clone()}
        if self._reward_type == "staged":
            info["reward_components"] = self._rc.clone()
        self._last_action = a
        return obs, reward, terminated, truncated, info

    # ------------------------------------------------------------------ expert + helpers
    def expert_plan(self, n_steps: int = ACTION_REPEAT) -> torch.Tensor:
        """PickAndPlaceTask.plan(n_steps) for all envs -> abs_pos actions [N, 4]."""
        self.sim.expert_plan(n_steps, self._expert_action.data_ptr())
        return self._expert_action.clone()

    def rollout_expert(self, n_env_steps: int):
        """Device-resident FSM rollout (generate_dataset.py:140-196), no host round trips."""
        self.sim.rollout_expert(n_env_steps)

    def _record_tensors(self, record, T: int, tables, always=()) -> dict:
        """The record of a rollout of T steps: `record` (a name or names) checked against `tables`, pairs of a
        field table {name: (width, dtype)} and the ctypes record that takes its arrays, then for those names and
        the missing ones of `always` behind them {name: tensor [T, N, width]} ([T, N] at width 1), each tensor's
        address stored in its record."""
        names = (record,) if isinstance(record, str) else tuple(record or ())
        allowed = tuple(name for fields, _ in tables for name in fields)
        for name in names:
            if name not in allowed:
                raise ValueError(f"record entries must be among {allowed}, got '{name}'")
        out = {}
        for name in names + tuple(n for n in always if n not in names):
            (width, dtype), rec = next((fields[name], rec) for fields, rec in tables if name in fields)
            shape = (T, self.num_envs, width) if width > 1 else (T, self.num_envs)
            out[name] = torch.empty(shape, dtype=getattr(torch, dtype), device=self.device)
            setattr(rec, name, out[name].data_ptr())
        return out

    def _check_bound(self, policy):
        """The policy's device side, given that it is bound to this env."""
        dev = policy.device_policy
        if policy.action_dim != self.action_dim or policy._env is not self:
            raise ValueError("the policy must be bound to this env (MlpPolicy.bind(env))")
        return dev

    def rollout(self, actions: torch.Tensor | None = None, n_steps: int | None = None,
                record=("obs", "reward", "done")) -> dict:
        """T env steps in fused launches with a per-step record, no host round trips.

        actions: [T, N, action_dim] fp32 on the GPU, one row per step and env (what T calls of step()
        would be given); None: n_steps steps of the on-device FSM expert (abs_pos envs).  Returns
        {name: tensor [T, N, ...]} for the names in `record` (_lib.TRAJ_FIELDS: obs, reward, done,
        reward_components, target, episode_i, qpos, qvel): slice k is what the env's buffer holds after
        step k, bit for bit what the step() loop gives ("obs" flat [T, N, 85]: split_obs; "done"
        int32 [T, N, 3] = terminated, truncated, success).  The env ends in the loop's final state."""
        if actions is None:
            if n_steps is None or int(n_steps) < 0:
                raise ValueError("rollout needs actions [T, N, A] or n_steps >= 0 for the on-device expert")
            T, a = int(n_steps), None
        else:
            a = torch.as_tensor(actions, dtype=torch.float32, device=self.device)
            if a.dim() != 3 or a.shape[1] != self.num_envs or a.shape[2] < self.action_dim:
                raise ValueError(f"actions must be [T, {self.num_envs}, {self.action_dim}], got {tuple(a.shape)}")
            if n_steps is not None and int(n_steps) != a.shape[0]:
                raise ValueError(f"n_steps {n_steps} does not match the {a.shape[0]} action rows")
            T, a = a.shape[0], a.contiguous()
        rec = _lib.MMXTrajectory()
        out = self._record_tensors(record, T, ((_lib.TRAJ_FIELDS, rec),))
        if T == 0:
            return out
        if a is None:
            self.sim.rollout_expert(T, rec)
        else:
            self.sim.rollout_actions(a.data_ptr(), a.shape[2], T, rec)
            self._last_action = a
        return out

    def rollout_policy(self, policy, n_steps: int, record=("obs", "reward", "done"), call: int = 0) -> dict:
        """n_steps closed-loop env steps under an MlpPolicy bound to this env (policy.MlpPolicy.bind), in the
        fused launches of rollout(): every env's wave evaluates the network on the observation the env holds
        (after an autoreset: the new episode's first) between two env steps.  Returns {name: tensor [T, N, ...]}
        for the names in `record`: the _lib.TRAJ_FIELDS entries as rollout() records them, always "actions"
        [T, N, action_dim] (what the envs were stepped with; rollout(actions=...) from the same state replays the
        call bit for bit), and on request "mean" (the network's output) and "noise" (the normal draws; increment
        `call` per call for fresh ones)."""
        own = {name: (self.action_dim, "float32") for name in ("actions", "mean", "noise")}
        if n_steps is None or int(n_steps) < 0:
            raise ValueError("rollout_policy needs n_steps >= 0")
        dev = self._check_bound(policy)
        T, rec, prec = int(n_steps), _lib.MMXTrajectory(), _lib.MMXPolicyRecord()
        out = self._record_tensors(record, T, ((_lib.TRAJ_FIELDS, rec), (own, prec)), always=("actions",))
        # (the policy's own arrays behind the env's, in the order of their record)
        out = {k: out[k] for k in [n for n in out if n not in own] + [n for n in own if n in out]}
        if T == 0:
            return out
        dev.rollout(self.sim, T, call, prec, rec)
        self._last_action = out["actions"]
        return out

    def rollout_dagger(self, policy, n_steps: int, beta: float = 0.5, takeover_dist: float = 0.0,
                       record=DAGGER_RECORD, call: int = 0) -> dict:
        """n_steps DAgger env steps (abs_pos envs) in the fused launches of rollout_policy: at every step the env's
        wave evaluates the bound MlpPolicy on the observation the env holds, the FSM expert plans beside it (at
        every step, whoever acts: its state shadows the learner's trajectory), and a gate picks the executed action:
        the expert's with probability `beta` per step and env (a Philox draw of (policy seed, call, step, env) that
        no noise component uses), and, with takeover_dist > 0, also wherever the learner's xyz target lies further
        than that from the expert's.  beta=1 is rollout(n_steps=...), beta=0 with takeover_dist=0 is
        rollout_policy.  Returns {name: tensor [T, N, ...]} for the names in `record`: the _lib.TRAJ_FIELDS entries
        as rollout() records them, always "actions" (what the envs were stepped with), and of _lib.DAGGER_FIELDS
        "expert_action" (the label: what expert_plan(16) returns at that state), "policy_action", "mean", "noise",
        "gate" (int32; bit 0 the draw, bit 1 the takeover; 0: the learner acted) and "obs_in" (the observation the
        learner was given: it pairs with the label; dagger.DaggerBuffer aggregates the pairs).  The env ends in the
        state of the loop expert_plan(16) -> step(actions[t]); increment `call` per call for fresh draws."""
        T, beta, takeover_dist, names = check_dagger_args(n_steps, beta, takeover_dist, record)
        dev = self._check_bound(policy)
        if self._action_mode != "abs_pos":
            raise ValueError("rollout_dagger needs action_mode abs_pos (the FSM expert's actions)")
        rec, drec = _lib.MMXTrajectory(), _lib.MMXDaggerRecord()
        out = self._record_tensors(names, T, ((_lib.TRAJ_FIELDS, rec), (_lib.DAGGER_FIELDS, drec)), always=("actions",))
        if T == 0:
            return out
        dev.rollout_dagger(self.sim, T, call, _lib.MMXDaggerConfig(beta=beta, takeover_dist=takeover_dist), drec, rec)
        self._last_action = out["actions"]
        return out

    # ------------------------------------------------------------------ advantages (mmx_gae)
    def gae(self, reward, done, value, value_last, gamma: float = 0.99, lam: float = 0.95, normalize: bool = False):
        """Generalised advantage estimation over a rollout record, on the env's stream: reward [T, N] float32, done
        [T, N, 3] int32 (a rollout's record), value [T, N] = V of the observation each step was given, value_last
        [N] = V of the observation after the last step (contiguous tensors on the env's device; N need not be
        num_envs).  Returns (adv, ret), both [T, N]: ret = adv + value before `normalize` rescales adv to mean 0 and
        variance 1 over all T N entries.  A terminated or truncated step takes next value 0 and cuts the recursion."""
        check_gae_args(reward, done, value, value_last, gamma, lam, self.device)
        T, N = reward.shape
        adv, ret = torch.empty_like(reward), torch.empty_like(reward)
        if T:
            cfg = _lib.MMXGaeConfig(gamma=float(gamma), lambda_=float(lam), normalize=int(bool(normalize)))
            with self.sim._on_sim_stream(self.device) as (cur, sst):
                for t in (reward, done, value, value_last, adv, ret):
                    t.record_stream(sst)
                self.sim.gae(cfg, T, N, reward.data_ptr(), done.data_ptr(), value.data_ptr(), value_last.data_ptr(),
                             adv.data_ptr(), ret.data_ptr())
        return adv, ret

    # ------------------------------------------------------------------ snapshot / restore
    def snapshot(self) -> Snapshot:
        """The state of every env, on the device (mmx_snapshot; asynchronous): everything a step reads and
        a reset / step returns, so a restored env continues bit for bit as this one does from here.  Not
        held: contacts and solver statistics of the last launch, the images (redrawn on restore), the
        dataset episode queue, the configuration."""
        data = torch.empty((self.num_envs, self.sim.snapshot_bytes), dtype=torch.uint8, device=self.device)
        self.sim.snapshot(data.data_ptr())
        return Snapshot(data)

    def restore(self, snap: Snapshot, src=None):
        """Put envs back to states of `snap`; returns (obs, info) like reset.  src None: env i takes record i
        (envs past the snapshot's last record are kept); an int: every env takes that record (the branch of
        a sampling planner); an int sequence or tensor [num_envs]: env i takes record src[i], -1 (or any
        index outside the snapshot) keeps env i as it is.  With cameras the restored envs are re-rendered.
        The snapshot may come from another env with the same record size (cameras or not); a different
        action mode, reward type or episode limit there is the caller's responsibility."""
        if not isinstance(snap, Snapshot):
            raise TypeError("restore needs a Snapshot (PickPlaceVecEnv.snapshot())")
        if snap.rec_bytes != self.sim.snapshot_bytes:
            raise ValueError(f"snapshot records have {snap.rec_bytes} bytes, this env's {self.sim.snapshot_bytes} "
                             "(a snapshot with cameras cannot go to an env without, or back)")
        if snap.data.device != self.device:
            raise ValueError(f"snapshot is on {snap.data.device}, this env on {self.device}")
        idx = None
        if src is not None:
            if isinstance(src, (int, np.integer)):
                idx = torch.full((self.num_envs,), int(src), dtype=torch.int32, device=self.device)
            else:
                idx = torch.as_tensor(src, device=self.device)
                if idx.dim() != 1 or idx.shape[0] != self.num_envs or idx.dtype.is_floating_point:
                    raise ValueError(f"src must be None, an int or {self.num_envs} ints, got shape {tuple(idx.shape)} "
                                     f"of {idx.dtype}")
                if idx.dtype != torch.int32:  # (an int64 index past 2^31 must not wrap into the snapshot)
                    idx = torch.where((idx >= 0) & (idx < snap.num_envs), idx, -1).to(torch.int32)
                idx = idx.contiguous()
        self.sim.restore(snap.data.data_ptr(), snap.num_envs, None if idx is None else idx.data_ptr())
        self._last_src = idx
        return self._obs_dict(), {}

    # ------------------------------------------------------------------ contact forces
    def contact_forces(self) -> dict:
        """Contacts and contact forces of every env's current state (mmx_contact_forces: the forward solve and
        mj_contactForce as a pass of its own; what data.contact, mujoco.mj_contactForce and data.qacc give in
        the reference after step()).  Valid after reset, step, any rollout (the final state) and restore; it
        changes nothing a step reads.  Returns torch tensors, views of sim-owned arrays that the next call
        overwrites (the launch is asynchronous on the env's stream, ordered like a step):
          contact [N, 64, 13]  dist, pos3, normal3, mu3, dim, geom1, geom2; zero past ncon
          force [N, 64, 5]     fn, the world-frame force on geom2's body (geom1's takes the opposite), the
                               torsional torque about the normal; zero past ncon
          body_wrench [N, 13, 6]  net contact force and torque about the body frame's origin (world) of bodies
                               _lib.FORCE_BODIES: links 2..8, hand 9, fingers 10, 11, cubes 16, 17, 18
          touch [N, 2]         per finger, the sum of fn over its contacts with cubes (the grip force)
          qacc [N, 27]         the solve's acceleration
          solve [N, 6]         _lib.FORCE_SOLVE_FIELDS: ncon, nefc, iterations, residual, exit, overflow
          geoms [N, 64, 2]     int64 geom1, geom2 (a copy; -1 past ncon)"""
        self.sim.contact_forces()
        out = dict(self.sim.force_views())
        ncon = out["solve"][:, 0].to(torch.int64)
        live = torch.arange(_lib.MAXCON, device=self.device)[None, :] < ncon[:, None]
        geoms = out["contact"][:, :, 11:13].to(torch.int64)
        out["geoms"] = torch.where(live[:, :, None], geoms, torch.full_like(geoms, -1))
        return out

    @property
    def step_count(self) -> torch.Tensor:
        return self._epi[:, _lib.EPI["step_count"]].clone()

    @property
    def tasks(self) -> list[tuple[str, str]]:
        ob = self._epi[:, 0].cpu().numpy()
        bn = self._epi[:, 1].cpu().numpy()
        return [(OBJECTS[o], BINS[b]) for o, b in zip(ob, bn)]

    @property
    def fsm_state(self) -> torch.Tensor:
        return self._epi[:, _lib.EPI["fsm_state"]].clone()

    @property
    def episode_flags(self) -> torch.Tensor:
        """staged-reward sticky flags: 1 grasped, 2 lifted, 4 above target, 8 placed"""
        return self._epi[:, _lib.EPI["flags"]].clone()

    @property
    def env_error(self) -> torch.Tensor:
        return self._epi[:, _lib.EPI["env_error"]].clone()

    @property
    def initial_ee_se3(self) -> torch.Tensor:
        T = torch.zeros(self.num_envs, 4, 4, device=self.device)
        f = self._epf
        T[:, :3, :3] = f[:, 0:9].reshape(-1, 3, 3)
        T[:, :3, 3] = f[:, 9:12]
        T[:, 3, 3] = 1.0
        return T

    def solver_stats(self) -> dict:
        s = self.stats.double().sum(dim=0).cpu().numpy()
        sub = max(s[3], 1.0)
        ks, kc = _lib.STAT_FIELDS.index("exit_stall"), _lib.STAT_FIELDS.index("exit_cap")
        out = {"mean_nefc": s[0] / sub, "mean_ncon": s[1] / sub, "mean_solver_iter": s[2] / sub,
               "max_resid": float(self.stats[:, 4].max().item()), "substeps": int(s[3]),
               # substeps whose Newton solve ended above the tolerance, by cause
               "exit_above_tol": {"no_progress": int(s[ks]), "iteration_cap": int(s[kc]),
                                  "fraction": float((s[ks] + s[kc]) / sub)}}
        # per-phase shader-clock cycles per substep per env (s_memtime ticks = shader cycles)
        for k, name in enumerate(_lib.STAT_FIELDS[5:17], start=5):
            out[name + "_per_substep"] = s[k] / sub
        return out

    def clear_stats(self):
        self.stats.zero_()

    def close(self):
        self.sim.close()
