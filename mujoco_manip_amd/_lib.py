"""ctypes binding of libmmx.so (include/mmx_api.h).

This is the reference-side binding a maintainer would add: the reference is Python, so the
binding to the C-ABI is ctypes.  Device buffers are exchanged as raw pointers; torch is used
only to own action tensors and to view sim-owned buffers (``__cuda_array_interface__``).
The product path fails loudly when the HIP library or the GPU is missing: there is no CPU
fallback.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

from . import _build

NQ, NV, NU, NOBS = 30, 27, 8, 85
MAXCON, CON_F = 64, 13
PNG_MAX_WIDTH = 10922  # include/mmx_api.h MMX_PNG_MAX_WIDTH
MMX_ESAMPLING = -4  # include/mmx_api.h: spawn sampling exhausted (randomization.py:84-87 raises RuntimeError)
# env_error bits (mujoco_manip_amd/csrc/mmx_state.h)
ERR_CON_OVERFLOW, ERR_EFC_OVERFLOW, ERR_NAN, ERR_SAMPLING = 1, 2, 4, 8
EPI_N, EPF_N, KIN_N, STAT_N = 18, 28, 63, 19
EPI_FIELDS = ("obj", "bin", "step_count", "flags", "fsm_state", "fsm_task_index", "fsm_settle", "fsm_gripper_open",
              "fsm_has_target", "env_error", "ncon", "nefc", "episodes", "rng_has32", "successes", "placed", "error_resets",
              "fsm_phases")
EPI = {name: k for k, name in enumerate(EPI_FIELDS)}
STAT_FIELDS = ("sum_nefc", "sum_ncon", "sum_solver_iter", "substeps", "max_resid", "cyc_ik", "cyc_kinematics",
               "cyc_dynamics", "cyc_collision", "cyc_constraints", "cyc_solver", "cyc_integrate", "cyc_step_end",
               "cyc_aux0", "cyc_aux1", "cyc_aux2", "cyc_aux3", "exit_stall", "exit_cap")
ACTION_MODES = ("abs_pos", "ee_pos_quat_g", "ee_pos_rot6d_g", "ee_pos_quat_g_rel", "ee_pos_rot6d_g_rel")
ACTION_DIMS = (4, 8, 10, 8, 10)
REWARD_TYPES = ("dense", "sparse", "staged")
# opt-in camera effects (include/mmx_api.h MMX_RENDER_SHADOWS, MMX_RENDER_TRANSLUCENT)
RENDER_EFFECTS = {"shadows": 1, "translucent_bins": 2}


def render_effect_flags(effects) -> int:
    """The flag mask of a tuple of effect names ("shadows", "translucent_bins"); () = 0."""
    if isinstance(effects, str):
        effects = (effects,)
    flags = 0
    for e in effects or ():
        if e not in RENDER_EFFECTS:
            raise ValueError(f"render_effects entries must be among {tuple(RENDER_EFFECTS)}, got '{e}'")
        flags |= RENDER_EFFECTS[e]
    return flags


class MMXConfig(C.Structure):
    _fields_ = [
        ("num_envs", C.c_int32), ("device", C.c_int32), ("action_mode", C.c_int32), ("reward_type", C.c_int32),
        ("max_episode_steps", C.c_int32), ("randomize_objects", C.c_int32),
        ("spawn_x_range", C.c_double * 2), ("spawn_y_range", C.c_double * 2),
        ("n_tasks", C.c_int32), ("task_obj", C.c_int8 * 9), ("task_bin", C.c_int8 * 9),
        ("fixed_task_obj", C.c_int32), ("fixed_task_bin", C.c_int32), ("image_size", C.c_int32),
        ("autoreset", C.c_int32), ("solver_iterations", C.c_int32), ("solver_tolerance", C.c_float),
        ("stream", C.c_void_p),
    ]


class MMXBuffers(C.Structure):
    _fields_ = [
        ("num_envs", C.c_int32), ("qpos", C.c_void_p), ("qvel", C.c_void_p), ("ctrl", C.c_void_p),
        ("qacc_warmstart", C.c_void_p), ("obs", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p),
        ("reward_components", C.c_void_p), ("episode_i", C.c_void_p), ("episode_f", C.c_void_p),
        ("kin", C.c_void_p), ("stats", C.c_void_p), ("contacts", C.c_void_p),
        ("images", C.c_void_p), ("seg", C.c_void_p), ("target", C.c_void_p),
    ]


class MMXForceBuffers(C.Structure):
    """mmx_force_buffers (include/mmx_api.h): the sim-owned outputs of the contact-force pass."""
    _fields_ = [
        ("num_envs", C.c_int32), ("contact", C.c_void_p), ("force", C.c_void_p), ("body_wrench", C.c_void_p),
        ("touch", C.c_void_p), ("qacc", C.c_void_p), ("solve", C.c_void_p),
    ]


# per-env shape of every array of mmx_force_buffers; the 13 moving bodies of body_wrench, in its order
FORCE_F, FORCE_SOLVE_F = 5, 6
FORCE_BODIES = (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18)
FORCE_SOLVE_FIELDS = ("ncon", "nefc", "iterations", "residual", "exit", "overflow")


class MMXTrajectory(C.Structure):
    """mmx_trajectory (include/mmx_api.h): caller-owned device arrays [T][N][F], NULL = not recorded."""
    _fields_ = [
        ("obs", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p), ("reward_components", C.c_void_p),
        ("target", C.c_void_p), ("episode_i", C.c_void_p), ("qpos", C.c_void_p), ("qvel", C.c_void_p),
    ]


MPPI_MAX_HORIZON, MPPI_MAX_ADIM = 64, 10  # include/mmx_api.h MMX_MPPI_MAX_HORIZON, MMX_MPPI_MAX_ADIM


class MMXMppiConfig(C.Structure):
    """mmx_mppi_config (include/mmx_api.h)."""
    _fields_ = [
        ("horizon", C.c_int32), ("samples", C.c_int32), ("temperature", C.c_float), ("discount", C.c_float),
        ("noise_beta", C.c_float), ("sigma", C.c_float * MPPI_MAX_ADIM), ("low", C.c_float * MPPI_MAX_ADIM),
        ("high", C.c_float * MPPI_MAX_ADIM), ("seed", C.c_uint64),
    ]


class MMXMppiBuffers(C.Structure):
    """mmx_mppi_buffers (include/mmx_api.h): planner-owned device arrays."""
    _fields_ = [
        ("nominal", C.c_void_p), ("noise", C.c_void_p), ("actions", C.c_void_p), ("reward", C.c_void_p),
        ("done", C.c_void_p), ("returns", C.c_void_p), ("weights", C.c_void_p), ("best", C.c_void_p),
    ]


# include/mmx_api.h MMX_POLICY_MAX_LAYERS, MMX_POLICY_MAX_WIDTH, MMX_POLICY_TANH / MMX_POLICY_RELU
POLICY_MAX_LAYERS, POLICY_MAX_WIDTH = 4, 256
POLICY_ACTIVATIONS = ("tanh", "relu")


class MMXPolicyConfig(C.Structure):
    """mmx_policy_config (include/mmx_api.h): host pointers, read during mmx_policy_create."""
    _fields_ = [
        ("n_layers", C.c_int32), ("width", C.c_int32 * POLICY_MAX_LAYERS), ("activation", C.c_int32),
        ("weight", C.c_void_p * POLICY_MAX_LAYERS), ("bias", C.c_void_p * POLICY_MAX_LAYERS),
        ("obs_shift", C.c_void_p), ("obs_scale", C.c_void_p), ("log_std", C.c_void_p), ("low", C.c_void_p),
        ("high", C.c_void_p), ("seed", C.c_uint64),
    ]


class MMXPolicyRecord(C.Structure):
    """mmx_policy_record (include/mmx_api.h): caller-owned device arrays [T][N][A]; actions is required."""
    _fields_ = [("actions", C.c_void_p), ("mean", C.c_void_p), ("noise", C.c_void_p)]


# include/mmx_api.h MMX_FIT_SGD / MMX_FIT_ADAM, MMX_FIT_MAX_BATCH
FIT_OPTIMIZERS = ("sgd", "adam")
FIT_MAX_BATCH = 65536


class MMXFitConfig(C.Structure):
    """mmx_fit_config (include/mmx_api.h): one mmx_policy_fit call's optimiser and batch selection."""
    _fields_ = [("optimizer", C.c_int32), ("batch", C.c_int32), ("shuffle", C.c_int32), ("reset_optimizer", C.c_int32),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("seed", C.c_uint64)]


class MMXGaeConfig(C.Structure):
    """mmx_gae_config (include/mmx_api.h): discount, lambda and whether mmx_gae normalises the advantages."""
    _fields_ = [("gamma", C.c_float), ("lambda_", C.c_float), ("normalize", C.c_int32)]


class MMXPgConfig(C.Structure):
    """mmx_pg_config (include/mmx_api.h): mmx_policy_fit's configuration and the surrogate's clip range."""
    _fields_ = [("fit", MMXFitConfig), ("clip", C.c_float)]


class MMXDaggerConfig(C.Structure):
    """mmx_dagger_config (include/mmx_api.h): the gate of mmx_rollout_dagger."""
    _fields_ = [("beta", C.c_float), ("takeover_dist", C.c_float)]


class MMXDaggerRecord(C.Structure):
    """mmx_dagger_record (include/mmx_api.h): caller-owned device arrays; actions is required."""
    _fields_ = [("actions", C.c_void_p), ("expert_action", C.c_void_p), ("policy_action", C.c_void_p), ("mean", C.c_void_p),
                ("noise", C.c_void_p), ("gate", C.c_void_p), ("obs_in", C.c_void_p)]


# per-env width and dtype of every array of a DAgger record
DAGGER_FIELDS = {"actions": (4, "float32"), "expert_action": (4, "float32"), "policy_action": (4, "float32"),
                 "mean": (4, "float32"), "noise": (4, "float32"), "gate": (1, "int32"), "obs_in": (NOBS, "float32")}


# per-env width and dtype of every trajectory array
TRAJ_FIELDS = {"obs": (NOBS, "float32"), "reward": (1, "float32"), "done": (3, "int32"),
               "reward_components": (6, "float32"), "target": (4, "float32"), "episode_i": (EPI_N, "int32"),
               "qpos": (NQ, "float32"), "qvel": (NV, "float32")}

# One env's snapshot record (include/mmx_api.h, mmx_snapshot / mmx_restore): (name, width, dtype) in the
# record's order; the fields are packed and the record padded to 16 bytes, rpose (cameras only) follows
RPOSE_N = 14 * 12  # body poses the cameras draw from: 14 slots x (R row-major 9, p 3)
SNAPSHOT_FIELDS = (("rng", 4, "uint64"), ("rng32", 1, "uint32"), ("qpos", NQ, "float32"), ("qvel", NV, "float32"),
                   ("ctrl", NU, "float32"), ("qacc_warmstart", NV, "float32"), ("kin", KIN_N, "float32"),
                   ("target", 4, "float32"), ("episode_i", EPI_N, "int32"), ("episode_f", EPF_N, "float32"),
                   ("obs", NOBS, "float32"), ("reward", 1, "float32"), ("reward_components", 6, "float32"),
                   ("done", 3, "int32"), ("rpose", RPOSE_N, "float32"))


def snapshot_record_bytes(cameras: bool) -> int:
    """Bytes of one record: the packed fields without rpose, padded to 16, then rpose with cameras."""
    fixed = sum(w * np.dtype(t).itemsize for name, w, t in SNAPSHOT_FIELDS if name != "rpose")
    return -(-fixed // 16) * 16 + (RPOSE_N * 4 if cameras else 0)


def snapshot_field_offsets(cameras: bool) -> dict:
    """{name: (byte offset, width, dtype)} of the fields of a record (a uint8 row of a Snapshot's tensor)."""
    out, off = {}, 0
    for name, w, t in SNAPSHOT_FIELDS:
        if name == "rpose":
            if not cameras:
                continue
            off = -(-off // 16) * 16
        out[name] = (off, w, t)
        off += w * np.dtype(t).itemsize
    return out


_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
_u8p, _i32p, _u64p, _fp = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
# Every C-ABI function, name -> (restype, argtypes), in the headers' order; load() applies it
_PROTOS = {
    # include/mmx_api.h
    "mmx_config_default": (None, [C.POINTER(MMXConfig)]),
    "mmx_create": (C.c_int, [C.POINTER(MMXConfig), C.POINTER(_vp)]),
    "mmx_destroy": (None, [_vp]),
    "mmx_last_error": (C.c_char_p, [_vp]),
    "mmx_reset": (C.c_int, [_vp, _u64p, _u8p, _i32p, _u8p]),
    "mmx_step": (C.c_int, [_vp, _vp, _i32]),
    "mmx_copy_ranges": (_i64, [_i64, _vp, _vp, _vp]),
    "mmx_expert_plan": (C.c_int, [_vp, _i32, _vp]),
    "mmx_rollout_expert": (C.c_int, [_vp, _i32]),
    "mmx_rollout_actions": (C.c_int, [_vp, _vp, _i32, _i32, C.POINTER(MMXTrajectory)]),
    "mmx_rollout_expert_record": (C.c_int, [_vp, _i32, C.POINTER(MMXTrajectory)]),
    "mmx_snapshot_bytes": (_i64, [_vp]),
    "mmx_snapshot": (C.c_int, [_vp, _vp, _i64]),
    "mmx_restore": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "mmx_mppi_create": (C.c_int, [_vp, C.POINTER(MMXMppiConfig), C.POINTER(_vp)]),
    "mmx_mppi_destroy": (None, [_vp]),
    "mmx_mppi_reset": (C.c_int, [_vp, _vp]),
    "mmx_mppi_plan": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "mmx_mppi_get_buffers": (C.c_int, [_vp, C.POINTER(MMXMppiBuffers)]),
    "mmx_mppi_reweight": (C.c_int, [_vp, _vp]),
    "mmx_policy_create": (C.c_int, [_vp, C.POINTER(MMXPolicyConfig), C.POINTER(_vp)]),
    "mmx_policy_destroy": (None, [_vp]),
    "mmx_policy_eval": (C.c_int, [_vp, _vp, _i32, _vp]),
    "mmx_rollout_policy": (C.c_int, [_vp, _vp, _i32, C.c_uint64, C.POINTER(MMXPolicyRecord), C.POINTER(MMXTrajectory)]),
    "mmx_policy_fit": (C.c_int, [_vp, _vp, _vp, _i64, _i32, C.POINTER(MMXFitConfig), _vp]),
    "mmx_policy_get_weights": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "mmx_policy_set_weights": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "mmx_gae": (C.c_int, [_vp, C.POINTER(MMXGaeConfig), _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mmx_policy_fit_pg": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, C.POINTER(MMXPgConfig), _vp]),
    "mmx_policy_set_log_std": (C.c_int, [_vp, _fp]),
    "mmx_rollout_dagger": (C.c_int, [_vp, _vp, _i32, C.c_uint64, C.POINTER(MMXDaggerConfig), C.POINTER(MMXDaggerRecord),
                                     C.POINTER(MMXTrajectory)]),
    "mmx_png_bound": (_i64, [_i32, _i32]),
    "mmx_png_scratch": (_i64, [_i32, _i32]),
    "mmx_png_encode": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "mmx_png_pack": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i32, _vp]),
    "mmx_image_stats": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "mmx_physics_step": (C.c_int, [_vp, _i32, _i32]),
    "mmx_forward": (C.c_int, [_vp]),
    "mmx_expert_physics": (C.c_int, [_vp, _i32]),
    "mmx_contact_forces": (C.c_int, [_vp]),
    "mmx_get_force_buffers": (C.c_int, [_vp, C.POINTER(MMXForceBuffers)]),
    "mmx_eval_reward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32]),
    "mmx_set_render_effects": (C.c_int, [_vp, _i32]),
    "mmx_get_render_effects": (C.c_int, [_vp]),
    "mmx_get_buffers": (C.c_int, [_vp, C.POINTER(MMXBuffers)]),
    "mmx_synchronize": (C.c_int, [_vp]),
    "mmx_get_state": (C.c_int, [_vp, _fp, _fp, _fp, _fp]),
    "mmx_set_state": (C.c_int, [_vp, _fp, _fp, _fp, _fp]),
    "mmx_queue_init": (C.c_int, [_vp, _i32, _u64p, _i32p]),
    "mmx_queue_advance": (C.c_int, [_vp, _vp, _vp]),
    "mmx_episode_seed": (C.c_uint32, [C.c_uint64, _i32]),
    # include/mmx_tuning.h
    "mmx_set_step_rows": (C.c_int, [_vp, _i32]),
    "mmx_step_rows": (C.c_int, [_vp]),
    "mmx_set_step_order": (C.c_int, [_vp, _i32]),
    "mmx_step_order": (C.c_int, [_vp]),
    "mmx_set_rollout_budget": (C.c_int, [_vp, _i32]),
    "mmx_rollout_budget": (C.c_int, [_vp]),
    "mmx_rollout_step_counts": (C.c_int, [_vp, _i32p, _i32p, _i32]),
    "mmx_rollout_launches": (C.c_int, [_vp, _i32]),
    "mmx_rollout_lanes": (C.c_int, [_vp]),
    "mmx_rollout_render_launches": (C.c_int, [_vp]),
    "mmx_rollout_render_overlap": (C.c_int, [_vp]),
    "mmx_rollout_steps_per_launch": (C.c_int, [_vp]),
    "mmx_kernel_timing": (C.c_int, [_vp, _i32]),
    "mmx_kernel_times": (C.c_int, [_vp, _fp, _i32p, _fp, _i32p]),
    "mmx_render_band_rows": (C.c_int, [C.c_int]),
    "mmx_render_bands_per_workgroup": (C.c_int, []),
}
EXPORTED = tuple(_PROTOS)

_default = None  # the handle load() gives without a path
_handles: dict = {}  # real path -> handle: a library is loaded and bound once


def load(path: str | None = None, build_if_missing: bool = True):
    """The bound handle of a build of the library, one per file.  Several may be loaded side by side (ctypes
    loads them RTLD_LOCAL: each resolves its own calls and keeps its own statics); a Sim uses the one it was
    created with (Sim(lib=...)).

    path None: the process's default, chosen once: MMX_LIB_PATH (a prebuilt variant of the same sources or a
    library of another revision, for every sim of the process: tools/ab.sh, tools/gpu.sh), else libmmx.so,
    or libmmx_prof.so with MMX_PROFILE=1, built in-tree by _build.build when missing and build_if_missing.
    The in-tree product and profile libraries must export every name of _PROTOS (__graft_entry__.build checks
    EXPORTED); any other library is bound with the names it has, and calling one it lacks is AttributeError."""
    global _default
    if path is None:
        if _default is None:
            profile = os.environ.get("MMX_PROFILE", "0") not in ("", "0")
            path = os.environ.get("MMX_LIB_PATH")
            if not path:
                path = _build.lib_path(profile)
                if not os.path.exists(path) and build_if_missing:
                    _build.build(profile=profile)
            _default = load(path)
        return _default
    real = os.path.realpath(path)
    if real not in _handles:
        if not os.path.exists(real):
            raise RuntimeError(f"{os.path.basename(path)} missing at {path}; run __graft_entry__.build()")
        L = C.CDLL(real)
        in_tree = real in (os.path.realpath(_build.LIB), os.path.realpath(_build.LIB_PROF))
        for name, (restype, argtypes) in _PROTOS.items():
            if in_tree or hasattr(L, name):
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
        _handles[real] = L
    return _handles[real]


def episode_seed(root: int, index: int) -> int:
    """SeedSequence(root).spawn(n)[index].generate_state(1)[0] (generate_dataset.py:263-268)."""
    return int(load().mmx_episode_seed(root, index))


class _DevArray:
    """Minimal __cuda_array_interface__ exporter for a sim-owned device buffer."""

    def __init__(self, ptr: int, shape, typestr: str, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}
        self._owner = owner


def _fptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


class _Owner:
    """Owner of one native object: `ptr`, created through the handle `L`, destroyed once by L's function DESTROY."""
    DESTROY = ""

    def close(self):
        if getattr(self, "ptr", None) is not None and self.ptr.value:
            getattr(self.L, self.DESTROY)(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Sim(_Owner):
    """Owner of one mmx_sim (a batch of num_envs environments on one GPU).  lib: the path of the build of the
    library that runs it (None: load()'s default); sims of different builds may be alive side by side."""
    DESTROY = "mmx_destroy"

    def __init__(self, num_envs: int, *, action_mode: str = "ee_pos_quat_g_rel", reward_type: str = "dense",
                 max_episode_steps: int = 500, randomize_objects: bool = False,
                 spawn_x_range=(-0.20, 0.20), spawn_y_range=(0.30, 0.45), task_pool=None, fixed_task=None,
                 image_size: int = 224, autoreset: bool = False, solver_iterations: int = 30,
                 solver_tolerance: float = 1e-6, device: int = 0, stream: int | None = None, render_effects=(),
                 lib: str | None = None):
        effects = render_effect_flags(render_effects)
        if effects and int(image_size) <= 0:
            raise ValueError("render_effects need cameras (image_size > 0)")
        if action_mode not in ACTION_MODES:
            raise ValueError(f"action_mode must be one of {ACTION_MODES}, got '{action_mode}'")
        if reward_type not in REWARD_TYPES:
            raise ValueError(f"reward_type must be one of {REWARD_TYPES}, got '{reward_type}'")
        if not (0 <= int(image_size) <= 1024):
            raise ValueError(f"image_size must be in [0, 1024] (0 = no cameras), got {image_size}")
        if int(num_envs) <= 0:
            raise ValueError(f"num_envs must be positive, got {num_envs}")
        self.L = load(lib)
        cfg = MMXConfig()
        self.L.mmx_config_default(C.byref(cfg))
        cfg.num_envs = int(num_envs)
        cfg.device = int(device)
        cfg.action_mode = ACTION_MODES.index(action_mode)
        cfg.reward_type = REWARD_TYPES.index(reward_type)
        cfg.max_episode_steps = int(max_episode_steps)
        cfg.randomize_objects = int(bool(randomize_objects))
        cfg.spawn_x_range[0], cfg.spawn_x_range[1] = spawn_x_range
        cfg.spawn_y_range[0], cfg.spawn_y_range[1] = spawn_y_range
        if task_pool is not None:
            cfg.n_tasks = len(task_pool)
            for k, (o, b) in enumerate(task_pool):
                cfg.task_obj[k], cfg.task_bin[k] = o, b
        if fixed_task is not None:
            cfg.fixed_task_obj, cfg.fixed_task_bin = fixed_task
        cfg.image_size = int(image_size)
        cfg.autoreset = int(bool(autoreset))
        cfg.solver_iterations = int(solver_iterations)
        cfg.solver_tolerance = float(solver_tolerance)
        cfg.stream = stream
        self.cfg = cfg
        self.num_envs = int(num_envs)
        self.action_dim = ACTION_DIMS[cfg.action_mode]
        ptr = C.c_void_p()
        rc = self.L.mmx_create(C.byref(cfg), C.byref(ptr))
        if rc != 0 or not ptr.value:
            raise RuntimeError(f"mmx_create failed ({rc}): no usable MI355X / HIP device?")
        self.ptr = ptr
        self.buffers = MMXBuffers()
        self._check(self.L.mmx_get_buffers(self.ptr, C.byref(self.buffers)), "mmx_get_buffers")
        if effects:  # before the first reset renders
            self.render_effects = effects

    def _check(self, rc, what):
        if rc == MMX_ESAMPLING:  # the reference's own exception and message (randomization.py:84-87)
            raise RuntimeError(self.L.mmx_last_error(self.ptr).decode())
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.L.mmx_last_error(self.ptr).decode()}")

    # ---- C-ABI calls
    def reset(self, seeds=None, task_override=None, env_mask=None):
        N = self.num_envs
        u64p, u8p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        s = g = t = m = None
        if seeds is not None:
            arr = np.zeros(N, np.uint64)
            given = np.zeros(N, np.uint8)
            for k, v in enumerate(seeds):
                if v is not None:
                    arr[k] = int(v)
                    given[k] = 1
            self._seed_arr, self._given_arr = arr, given
            s, g = arr.ctypes.data_as(u64p), given.ctypes.data_as(u8p)
        if task_override is not None:
            self._task_arr = np.ascontiguousarray(task_override, np.int32)
            t = self._task_arr.ctypes.data_as(i32p)
        if env_mask is not None:
            self._mask_arr = np.ascontiguousarray(env_mask, np.uint8)
            m = self._mask_arr.ctypes.data_as(u8p)
        self._check(self.L.mmx_reset(self.ptr, s, g, t, m), "mmx_reset")

    def queue_init(self, tasks, seeds=None):
        """Device-side episode queue (mmx_queue_init): tasks[e] = obj << 4 | bin of episode e and,
        optionally, its seed (PCG64(SeedSequence(seed)) at its reset)."""
        t = np.ascontiguousarray(tasks, np.int32)
        s = None if seeds is None else np.ascontiguousarray([int(v) for v in seeds], np.uint64)
        if s is not None and len(s) != len(t):
            raise ValueError("seeds and tasks must have one entry per episode")
        self._check(self.L.mmx_queue_init(self.ptr, len(t), None if s is None else s.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          t.ctypes.data_as(C.POINTER(C.c_int32))), "mmx_queue_init")

    def queue_advance(self, slot_ep_ptr: int | None = None, fin_ep_ptr: int | None = None):
        """Hand the next episodes to the free / finished slots and reset them (mmx_queue_advance;
        asynchronous).  The pointers: device int32 [N] outputs (slot -> episode after the call,
        episode that ended in the slot at this call; -1 = none)."""
        self._check(self.L.mmx_queue_advance(self.ptr, C.c_void_p(slot_ep_ptr) if slot_ep_ptr else None,
                                             C.c_void_p(fin_ep_ptr) if fin_ep_ptr else None), "mmx_queue_advance")

    def step(self, action_ptr: int, action_dim: int):
        self._check(self.L.mmx_step(self.ptr, C.c_void_p(action_ptr), action_dim), "mmx_step")

    def expert_plan(self, n_steps: int, action_ptr: int | None):
        self._check(self.L.mmx_expert_plan(self.ptr, n_steps, C.c_void_p(action_ptr) if action_ptr else None),
                    "mmx_expert_plan")

    def rollout_expert(self, n_env_steps: int, record: MMXTrajectory | None = None):
        """n_env_steps of the on-device expert; `record`: device arrays [T][N][F] that receive every step's outputs."""
        if record is None:
            self._check(self.L.mmx_rollout_expert(self.ptr, n_env_steps), "mmx_rollout_expert")
        else:
            self._check(self.L.mmx_rollout_expert_record(self.ptr, n_env_steps, C.byref(record)), "mmx_rollout_expert_record")

    def rollout_actions(self, actions_ptr: int, action_dim: int, n_env_steps: int, record: MMXTrajectory | None = None):
        """n_env_steps through the device actions [T][N][action_dim] in fused launches (mmx_rollout_actions)."""
        self._check(self.L.mmx_rollout_actions(self.ptr, C.c_void_p(actions_ptr), action_dim, n_env_steps,
                                               None if record is None else C.byref(record)), "mmx_rollout_actions")

    @property
    def snapshot_bytes(self) -> int:
        """Bytes of one env's snapshot record for this sim (mmx_snapshot_bytes: larger with cameras)."""
        return int(self.L.mmx_snapshot_bytes(self.ptr))

    def snapshot(self, ptr: int):
        """Write every env's record to device memory at `ptr` (num_envs * snapshot_bytes bytes, 16-byte
        aligned): record i = env i (mmx_snapshot; asynchronous on the sim's stream)."""
        self._check(self.L.mmx_snapshot(self.ptr, C.c_void_p(ptr), self.snapshot_bytes), "mmx_snapshot")

    def restore(self, ptr: int, n_records: int, src_ptr: int | None = None):
        """Env i takes record src[i] of the n_records records at `ptr` (src_ptr: device int32 [num_envs];
        an index outside [0, n_records) keeps the env; None: env i takes record i where there is one);
        with cameras the restored envs are re-rendered (mmx_restore; asynchronous on the sim's stream)."""
        self._check(self.L.mmx_restore(self.ptr, C.c_void_p(ptr), self.snapshot_bytes, int(n_records),
                                       C.c_void_p(src_ptr) if src_ptr else None), "mmx_restore")

    def kernel_timing(self, enable: bool):
        """Start (True: a new collection) / stop bracketing every rollout launch with HIP events."""
        self._check(self.L.mmx_kernel_timing(self.ptr, int(bool(enable))), "mmx_kernel_timing")

    def kernel_times(self) -> dict:
        """Summed launch durations (ms) and launch counts since kernel_timing(True); waits for them."""
        sm, rm, sn, rn = C.c_float(), C.c_float(), C.c_int32(), C.c_int32()
        self._check(self.L.mmx_kernel_times(self.ptr, C.byref(sm), C.byref(sn), C.byref(rm), C.byref(rn)),
                    "mmx_kernel_times")
        return {"step_ms": sm.value, "step_launches": sn.value, "render_ms": rm.value, "render_launches": rn.value}

    @contextlib.contextmanager
    def _on_sim_stream(self, device):
        """Run the body on the sim's stream (the encoder and the statistics kernel launch there),
        ordered after the caller's current stream; on exit the caller's stream waits for the body,
        whatever stream the caller is on.  Yields (caller's stream, sim's stream)."""
        import torch

        cur = torch.cuda.current_stream(device)
        sst = (torch.cuda.ExternalStream(self.cfg.stream, device=device) if self.cfg.stream
               else torch.cuda.default_stream(device))
        sst.wait_stream(cur)
        with torch.cuda.stream(sst):
            yield cur, sst
        cur.wait_stream(sst)

    def _png_encode_pack(self, ptr, stride, n, W, H, bound, scr, dev, exact):
        """mmx_png_encode of n images from `ptr` (`stride` bytes apart), then the files packed back
        to back (mmx_png_pack) -> (packed, ends int64 [n]), on the current stream.  exact: packed
        has exactly the files' bytes (a host synchronisation for the size); else room for n * bound."""
        import torch

        out = torch.empty(n * bound, dtype=torch.uint8, device=dev)
        scratch = torch.empty(n * scr, dtype=torch.uint8, device=dev)
        sizes = torch.empty(n, dtype=torch.int32, device=dev)
        self._check(self.L.mmx_png_encode(self.ptr, C.c_void_p(ptr), stride, n, W, H, C.c_void_p(out.data_ptr()), bound,
                                          C.c_void_p(sizes.data_ptr()), C.c_void_p(scratch.data_ptr())), "mmx_png_encode")
        ends = torch.cumsum(sizes.to(torch.int64), 0)
        starts = ends - sizes.to(torch.int64)
        packed = torch.empty(int(ends[-1].item()) if exact else n * bound, dtype=torch.uint8, device=dev)
        self._check(self.L.mmx_png_pack(self.ptr, C.c_void_p(out.data_ptr()), bound, C.c_void_p(sizes.data_ptr()),
                                        C.c_void_p(starts.data_ptr()), n, C.c_void_p(packed.data_ptr())), "mmx_png_pack")
        return packed, ends

    def png_encode(self, images, max_batch: int = 4096):
        """PNG files of RGB8 images [n, H, W, 3] (a CUDA uint8 tensor, any row-contiguous layout)
        encoded on the device (mmx_png_encode), in batches of `max_batch`.  Returns (packed uint8
        CUDA tensor, int64 offsets [n + 1] on the host): file i is packed[offsets[i]:offsets[i + 1]].
        One host synchronisation per batch (the packed size)."""
        import torch

        n, H, W, c = images.shape
        assert c == 3 and images.dtype == torch.uint8 and images.is_cuda
        if n == 0:
            return torch.empty(0, dtype=torch.uint8, device=images.device), np.zeros(1, np.int64)
        bound, scr = int(self.L.mmx_png_bound(W, H)), int(self.L.mmx_png_scratch(W, H))
        if bound < 0:
            raise ValueError(f"unsupported image size {W} x {H}")
        with self._on_sim_stream(images.device) as (cur, sst):  # the buffers, the size scan and the read-back too
            imgs = images.contiguous()
            images.record_stream(sst)
            parts, offs = [], [0]
            for b0 in range(0, n, max_batch):
                m = min(max_batch, n - b0)
                packed, ends = self._png_encode_pack(imgs[b0].data_ptr(), H * W * 3, m, W, H, bound, scr, imgs.device, True)
                parts.append(packed)
                offs.extend((ends.cpu().numpy() + offs[-1]).tolist())
            packed = torch.cat(parts) if len(parts) > 1 else parts[0]
        packed.record_stream(cur)
        return packed, np.asarray(offs, np.int64)

    def png_encode_device(self, images):
        """PNG files of RGB8 images [n, H, W, 3] (CUDA uint8, rows contiguous) encoded and packed on
        the device with NO host synchronisation: returns (packed, ends), both CUDA tensors on the
        caller's stream: file i is packed[ends[i - 1]:ends[i]] (ends int64 [n]); packed has room for
        n * mmx_png_bound bytes, of which the first ends[-1] are files.  The dataset loop copies
        the sizes and the packed bytes to the host asynchronously."""
        import torch

        n, H, W, c = images.shape
        assert c == 3 and images.dtype == torch.uint8 and images.is_cuda and n > 0
        assert images.stride(1) == W * 3 and images.stride(2) == 3 and images.stride(3) == 1, "rows must be contiguous"
        bound, scr = int(self.L.mmx_png_bound(W, H)), int(self.L.mmx_png_scratch(W, H))
        if bound < 0:
            raise ValueError(f"unsupported image size {W} x {H}")
        with self._on_sim_stream(images.device) as (cur, sst):
            images.record_stream(sst)
            packed, ends = self._png_encode_pack(images.data_ptr(), images.stride(0), n, W, H, bound, scr, images.device,
                                                 False)
        packed.record_stream(cur)
        ends.record_stream(cur)
        return packed, ends

    def image_stats(self, images):
        """Per-image channel statistics of RGB8 images [n, H, W, 3] (CUDA uint8, rows contiguous, any
        stride between images) on the device, asynchronously on the caller's stream: int64 [n, 4, 3]
        = (min, max, sum, sum of squares) x (R, G, B) over every pixel (mmx_image_stats)."""
        import torch

        n, H, W, c = images.shape
        assert c == 3 and images.dtype == torch.uint8 and images.is_cuda
        assert images.stride(1) == W * 3 and images.stride(2) == 3 and images.stride(3) == 1, "rows must be contiguous"
        out = torch.empty((n, 4, 3), dtype=torch.int64, device=images.device)
        if n == 0:
            return out
        with self._on_sim_stream(images.device) as (_, sst):
            images.record_stream(sst)
            out.record_stream(sst)
            self._check(self.L.mmx_image_stats(self.ptr, C.c_void_p(images.data_ptr()), images.stride(0), n, W, H,
                                               C.c_void_p(out.data_ptr())), "mmx_image_stats")
        return out

    @property
    def rollout_lanes(self) -> int:
        return int(self.L.mmx_rollout_lanes(self.ptr))

    @property
    def rollout_render_launches(self) -> int:
        """Render launches per rollout step with cameras (1: one over all envs after every lane's step)."""
        return int(self.L.mmx_rollout_render_launches(self.ptr))

    @property
    def step_rows(self) -> int:
        """Constraint rows the env-step kernel keeps in LDS (128: twelve envs per CU; 192: four, each
        with a helper wave; chosen at create from the batch size)."""
        return int(self.L.mmx_step_rows(self.ptr))

    @step_rows.setter
    def step_rows(self, rows: int):
        self._check(self.L.mmx_set_step_rows(self.ptr, int(rows)), "mmx_set_step_rows")

    @property
    def render_effects(self) -> int:
        """Flag mask of the opt-in camera effects (RENDER_EFFECTS: cast shadows, translucent bins; 0 =
        the default flat images).  Setting it takes effect from the next render."""
        return int(self.L.mmx_get_render_effects(self.ptr))

    @render_effects.setter
    def render_effects(self, flags):
        if not isinstance(flags, int):
            flags = render_effect_flags(flags)
        self._check(self.L.mmx_set_render_effects(self.ptr, int(flags)), "mmx_set_render_effects")

    @property
    def rollout_render_overlap(self) -> bool:
        """Camera rollouts render step k beside the env-step launch of step k + 1 (timing only)."""
        return bool(self.L.mmx_rollout_render_overlap(self.ptr))

    @property
    def step_order(self) -> bool:
        """Env-step launches dispatch their envs longest first by FSM phase (True, the default) or in
        index order; results are bit-identical either way."""
        return bool(self.L.mmx_step_order(self.ptr))

    @step_order.setter
    def step_order(self, on: bool):
        self._check(self.L.mmx_set_step_order(self.ptr, 1 if on else 0), "mmx_set_step_order")

    @property
    def rollout_budget(self) -> bool:
        """rollout_expert's launches stop by the clock (True, the default where it applies: 128 rows, no
        cameras, at least 6 launches per lane) or after fixed step counts; results are bit-identical either way."""
        return bool(self.L.mmx_rollout_budget(self.ptr))

    @rollout_budget.setter
    def rollout_budget(self, on: bool):
        self._check(self.L.mmx_set_rollout_budget(self.ptr, 1 if on else 0), "mmx_set_rollout_budget")

    def rollout_step_counts(self, log_launches: int = 0):
        """The env steps each env made in the last budgeted rollout_expert call (int32 [N]; waits for the sim's
        stream), and with log_launches = MMX_ROLLOUT_LOG of the sim's creation also the counts after each
        launch of the env's lane (int32 [log_launches, N])."""
        out = np.zeros(self.num_envs, np.int32)
        log = np.zeros((log_launches, self.num_envs), np.int32) if log_launches else None
        self._check(self.L.mmx_rollout_step_counts(self.ptr, out.ctypes.data_as(_i32p),
                                                   log.ctypes.data_as(_i32p) if log_launches else None, log_launches),
                    "mmx_rollout_step_counts")
        return (out, log) if log_launches else out

    @property
    def rollout_steps_per_launch(self) -> int:
        return int(self.L.mmx_rollout_steps_per_launch(self.ptr))

    def rollout_launches(self, n_env_steps: int) -> int:
        """Launches per rollout lane that rollout_expert(n_env_steps) makes."""
        return int(self.L.mmx_rollout_launches(self.ptr, int(n_env_steps)))

    def physics_step(self, n: int = 1, with_ik: bool = False):
        self._check(self.L.mmx_physics_step(self.ptr, n, int(with_ik)), "mmx_physics_step")

    def forward(self):
        self._check(self.L.mmx_forward(self.ptr), "mmx_forward")

    def expert_physics(self, n_physics_steps: int):
        """n x (PickAndPlaceTask.update() ; mj_step), main.py:65-91."""
        self._check(self.L.mmx_expert_physics(self.ptr, n_physics_steps), "mmx_expert_physics")

    def eval_reward(self, obj_ptr: int, ee_ptr: int, ctrl7_ptr: int, pairs_ptr: int | None, max_pairs: int):
        """Reward-layer harness (device pointers): _compute_reward at the given positions / contacts."""
        self._check(self.L.mmx_eval_reward(self.ptr, C.c_void_p(obj_ptr), C.c_void_p(ee_ptr), C.c_void_p(ctrl7_ptr),
                                           C.c_void_p(pairs_ptr) if pairs_ptr else None, max_pairs),
                    "mmx_eval_reward")

    def contact_forces(self):
        """The contact-force pass on the current state of every env (mmx_contact_forces; asynchronous on the
        sim's stream): the forward solve and mj_contactForce into the arrays of force_views()."""
        self._check(self.L.mmx_contact_forces(self.ptr), "mmx_contact_forces")

    def gae(self, cfg: "MMXGaeConfig", T: int, N: int, reward_ptr: int, done_ptr: int, value_ptr: int, value_last_ptr: int,
            adv_ptr: int, ret_ptr: int | None = None):
        """GAE(lambda) over a [T][N] record into adv (and ret) at the device pointers (mmx_gae; asynchronous on the
        sim's stream)."""
        self._check(self.L.mmx_gae(self.ptr, C.byref(cfg), int(T), int(N), C.c_void_p(reward_ptr), C.c_void_p(done_ptr),
                                   C.c_void_p(value_ptr), C.c_void_p(value_last_ptr), C.c_void_p(adv_ptr),
                                   C.c_void_p(ret_ptr) if ret_ptr else None), "mmx_gae")

    def force_views(self) -> dict:
        """Zero-copy torch views of the contact-force pass's outputs (mmx_force_buffers), valid until the sim
        closes; they exist from the first contact_forces() call on."""
        import torch

        if getattr(self, "_force_buffers", None) is None:
            b = MMXForceBuffers()
            self._check(self.L.mmx_get_force_buffers(self.ptr, C.byref(b)), "mmx_get_force_buffers")
            self._force_buffers = b
        b, N, dev = self._force_buffers, self.num_envs, f"cuda:{self.cfg.device}"
        shapes = {"contact": (N, MAXCON, CON_F), "force": (N, MAXCON, FORCE_F), "body_wrench": (N, len(FORCE_BODIES), 6),
                  "touch": (N, 2), "qacc": (N, NV), "solve": (N, FORCE_SOLVE_F)}
        return {n: torch.as_tensor(_DevArray(getattr(b, n), shp, "<f4", self), device=dev) for n, shp in shapes.items()}

    def synchronize(self):
        self._check(self.L.mmx_synchronize(self.ptr), "mmx_synchronize")

    def get_state(self):
        N = self.num_envs
        qpos, qvel = np.zeros((N, NQ), np.float32), np.zeros((N, NV), np.float32)
        ctrl, ws = np.zeros((N, NU), np.float32), np.zeros((N, NV), np.float32)
        self._check(self.L.mmx_get_state(self.ptr, _fptr(qpos), _fptr(qvel), _fptr(ctrl), _fptr(ws)), "mmx_get_state")
        return qpos, qvel, ctrl, ws

    def set_state(self, qpos=None, qvel=None, ctrl=None, qacc_ws=None):
        arrs = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (qpos, qvel, ctrl, qacc_ws)]
        self._check(self.L.mmx_set_state(self.ptr, *[_fptr(a) for a in arrs]), "mmx_set_state")

    # ---- zero-copy torch views of sim-owned buffers (env-major [N][F])
    def image_views(self):
        """(rgb [N, 2, S, S, 3] uint8, seg [N, 2, S, S] uint8) or None when image_size == 0."""
        import torch

        S = int(self.cfg.image_size)
        if S <= 0 or not self.buffers.images:
            return None
        dev = f"cuda:{self.cfg.device}"
        rgb = torch.as_tensor(_DevArray(self.buffers.images, (self.num_envs, 2, S, S, 3), "|u1", self), device=dev)
        seg = torch.as_tensor(_DevArray(self.buffers.seg, (self.num_envs, 2, S, S), "|u1", self), device=dev)
        return rgb, seg

    def view(self, name: str, nfield: int, dtype: str = "<f4"):
        import torch

        ptr = getattr(self.buffers, name)
        shape = (self.num_envs, nfield) if nfield > 1 else (self.num_envs,)
        return torch.as_tensor(_DevArray(ptr, shape, dtype, self), device=f"cuda:{self.cfg.device}")


class Mppi(_Owner):
    """Owner of one mmx_mppi bound to a camera-less planner Sim of M * samples envs (mmx_mppi_* of
    include/mmx_api.h).  Close it before the planner sim."""
    DESTROY = "mmx_mppi_destroy"

    def __init__(self, sim: Sim, *, horizon: int, samples: int, sigma, low, high, temperature: float = 1.0,
                 discount: float = 1.0, noise_beta: float = 0.0, seed: int = 0):
        A = sim.action_dim
        for name, v in (("sigma", sigma), ("low", low), ("high", high)):
            if len(v) != A:
                raise ValueError(f"{name} must have {A} entries (the action dimension), got {len(v)}")
        cfg = MMXMppiConfig(horizon=int(horizon), samples=int(samples), temperature=float(temperature),
                            discount=float(discount), noise_beta=float(noise_beta), seed=int(seed) & (2**64 - 1))
        for a in range(A):
            cfg.sigma[a], cfg.low[a], cfg.high[a] = float(sigma[a]), float(low[a]), float(high[a])
        self.sim, self.cfg, self.L = sim, cfg, sim.L
        self.H, self.K, self.A = int(horizon), int(samples), A
        ptr = C.c_void_p()
        rc = self.L.mmx_mppi_create(sim.ptr, C.byref(cfg), C.byref(ptr))
        if rc != 0 or not ptr.value:
            raise ValueError(f"mmx_mppi_create failed ({rc}): {self.L.mmx_last_error(sim.ptr).decode()}")
        self.ptr = ptr
        self.M = sim.num_envs // self.K
        self.buffers = MMXMppiBuffers()
        sim._check(self.L.mmx_mppi_get_buffers(self.ptr, C.byref(self.buffers)), "mmx_mppi_get_buffers")

    def reset(self, action_ptr: int):
        """Every step of every nominal plan = the device action [M][A]; the call counter to 0 (mmx_mppi_reset)."""
        self.sim._check(self.L.mmx_mppi_reset(self.ptr, C.c_void_p(action_ptr)), "mmx_mppi_reset")

    def plan(self, snap_ptr: int, rec_bytes: int, n_records: int, xi_ptr: int | None, out_ptr: int):
        """One control step for the M records at snap_ptr -> the device action [M][A] at out_ptr (mmx_mppi_plan;
        asynchronous on the planner sim's stream)."""
        self.sim._check(self.L.mmx_mppi_plan(self.ptr, C.c_void_p(snap_ptr), int(rec_bytes), int(n_records),
                                             C.c_void_p(xi_ptr) if xi_ptr else None, C.c_void_p(out_ptr)), "mmx_mppi_plan")

    def reweight(self, out_ptr: int):
        """The reweight pass alone on the planner's arrays as they stand (mmx_mppi_reweight: a test harness)."""
        self.sim._check(self.L.mmx_mppi_reweight(self.ptr, C.c_void_p(out_ptr)), "mmx_mppi_reweight")

    def views(self) -> dict:
        """Zero-copy torch views of the planner-owned arrays (mmx_mppi_buffers)."""
        import torch

        H, M, K, A, N = self.H, self.M, self.K, self.A, self.M * self.K
        shapes = {"nominal": ((H, M, A), "<f4"), "noise": ((H, N, A), "<f4"), "actions": ((H, N, A), "<f4"),
                  "reward": ((H, N), "<f4"), "done": ((H, N, 3), "<i4"), "returns": ((N,), "<f4"),
                  "weights": ((N,), "<f4"), "best": ((M,), "<i4")}
        dev = f"cuda:{self.sim.cfg.device}"
        return {n: torch.as_tensor(_DevArray(getattr(self.buffers, n), shp, t, self), device=dev)
                for n, (shp, t) in shapes.items()}


class Policy(_Owner):
    """Owner of one mmx_policy on the device of `sim` (mmx_policy_* of include/mmx_api.h): an MLP on the numeric
    observation.  layers: [(W [out, in], b [out] or None), ...] float32 numpy arrays; the other arrays float32 or
    None.  Close it before the sim."""
    DESTROY = "mmx_policy_destroy"

    def __init__(self, sim: Sim, layers, activation: int, obs_shift=None, obs_scale=None, log_std=None, low=None,
                 high=None, seed: int = 0):
        cfg = MMXPolicyConfig(n_layers=len(layers), activation=int(activation), seed=int(seed) & (2**64 - 1))
        keep = []  # the host arrays, alive during the call

        def ptr(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float32)
            keep.append(a)
            return a.ctypes.data

        for k, (W, b) in enumerate(layers[:POLICY_MAX_LAYERS]):
            cfg.width[k] = int(np.shape(W)[0])
            cfg.weight[k], cfg.bias[k] = ptr(W), ptr(b)
        cfg.obs_shift, cfg.obs_scale, cfg.log_std = ptr(obs_shift), ptr(obs_scale), ptr(log_std)
        cfg.low, cfg.high = ptr(low), ptr(high)
        self.sim, self.L = sim, sim.L
        self.action_dim = int(np.shape(layers[-1][0])[0]) if layers else 0
        self.shapes = [tuple(int(v) for v in np.shape(W)) for W, _ in layers]  # [(out, in), ...]
        out = C.c_void_p()
        rc = self.L.mmx_policy_create(sim.ptr, C.byref(cfg), C.byref(out))
        if rc != 0 or not out.value:
            raise ValueError(f"mmx_policy_create failed ({rc}): {self.L.mmx_last_error(sim.ptr).decode()}")
        self.ptr = out

    def eval(self, obs_ptr: int, n: int, out_ptr: int):
        """mean [n][A] at out_ptr of the observations [n][85] at obs_ptr (device pointers; mmx_policy_eval,
        asynchronous on the creating sim's stream)."""
        self.sim._check(self.L.mmx_policy_eval(self.ptr, C.c_void_p(obs_ptr), int(n), C.c_void_p(out_ptr)), "mmx_policy_eval")

    def fit(self, obs_ptr: int, target_ptr: int, n_pairs: int, n_steps: int, cfg: MMXFitConfig, loss_ptr: int | None = None):
        """n_steps optimisation steps on the pairs (obs [n][85], target [n][A]: device pointers) that update the
        weights in place; loss_ptr: device [n_steps] or None (mmx_policy_fit, asynchronous on the creating sim's
        stream)."""
        self.sim._check(self.L.mmx_policy_fit(self.ptr, C.c_void_p(obs_ptr), C.c_void_p(target_ptr), int(n_pairs), int(n_steps),
                                              C.byref(cfg), C.c_void_p(loss_ptr) if loss_ptr else None), "mmx_policy_fit")

    def fit_pg(self, obs_ptr: int, mean_old_ptr: int, noise_ptr: int, adv_ptr: int, n_pairs: int, n_steps: int, cfg: MMXPgConfig,
               stats_ptr: int | None = None):
        """n_steps steps of PPO's clipped surrogate on the samples (obs [n][85], mean_old and noise [n][A], adv [n]:
        device pointers) that update the weights in place; stats_ptr: device [n_steps][3] or None (mmx_policy_fit_pg,
        asynchronous on the creating sim's stream)."""
        self.sim._check(self.L.mmx_policy_fit_pg(self.ptr, C.c_void_p(obs_ptr), C.c_void_p(mean_old_ptr), C.c_void_p(noise_ptr),
                                                 C.c_void_p(adv_ptr), int(n_pairs), int(n_steps), C.byref(cfg),
                                                 C.c_void_p(stats_ptr) if stats_ptr else None), "mmx_policy_fit_pg")

    def set_log_std(self, log_std):
        """std = exp(log_std [A]) into the device blob, in place (mmx_policy_set_log_std)."""
        a = np.ascontiguousarray(log_std, np.float32)
        self.sim._check(self.L.mmx_policy_set_log_std(self.ptr, a.ctypes.data_as(_fp)), "mmx_policy_set_log_std")

    def get_weights(self) -> list:
        """[(W [out, in], b [out]), ...] float32 numpy arrays of the weights as they are now (mmx_policy_get_weights;
        synchronises the creating sim's stream)."""
        layers = [(np.empty(shp, np.float32), np.empty(shp[0], np.float32)) for shp in self.shapes]
        wp = (C.c_void_p * POLICY_MAX_LAYERS)(*[W.ctypes.data for W, _ in layers])
        bp = (C.c_void_p * POLICY_MAX_LAYERS)(*[b.ctypes.data for _, b in layers])
        self.sim._check(self.L.mmx_policy_get_weights(self.ptr, wp, bp), "mmx_policy_get_weights")
        return layers

    def set_weights(self, layers):
        """The reverse: layers [(W [out, in], b [out] or None), ...] of the policy's own shapes into the device
        blob, in place (mmx_policy_set_weights); the optimiser's state stays."""
        if len(layers) != len(self.shapes):
            raise ValueError(f"the policy has {len(self.shapes)} layers, got {len(layers)}")
        keep = []
        for k, ((W, b), shp) in enumerate(zip(layers, self.shapes)):
            if tuple(np.shape(W)) != shp or (b is not None and tuple(np.shape(b)) != (shp[0],)):
                raise ValueError(f"layers[{k}] must be ([{shp[0]}, {shp[1]}], [{shp[0]}] or None)")
            keep.append((np.ascontiguousarray(W, np.float32), None if b is None else np.ascontiguousarray(b, np.float32)))
        wp = (C.c_void_p * POLICY_MAX_LAYERS)(*[W.ctypes.data for W, _ in keep])
        bp = (C.c_void_p * POLICY_MAX_LAYERS)(*[None if b is None else b.ctypes.data for _, b in keep])
        self.sim._check(self.L.mmx_policy_set_weights(self.ptr, wp, bp), "mmx_policy_set_weights")

    def rollout(self, sim: Sim, n_env_steps: int, call: int, prec: MMXPolicyRecord, record: MMXTrajectory | None = None):
        """n_env_steps closed-loop env steps of `sim` under this policy in fused launches (mmx_rollout_policy)."""
        sim._check(self.L.mmx_rollout_policy(sim.ptr, self.ptr, int(n_env_steps), int(call) & (2**64 - 1), C.byref(prec),
                                             None if record is None else C.byref(record)), "mmx_rollout_policy")

    def rollout_dagger(self, sim: Sim, n_env_steps: int, call: int, cfg: MMXDaggerConfig, drec: MMXDaggerRecord,
                       record: MMXTrajectory | None = None):
        """n_env_steps env steps of `sim` under this policy or the FSM expert, by the gate of cfg, with the expert's
        label recorded at every step (mmx_rollout_dagger)."""
        sim._check(self.L.mmx_rollout_dagger(sim.ptr, self.ptr, int(n_env_steps), int(call) & (2**64 - 1), C.byref(cfg),
                                             C.byref(drec), None if record is None else C.byref(record)), "mmx_rollout_dagger")
