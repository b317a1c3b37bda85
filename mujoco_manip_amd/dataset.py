"""Batched expert-demonstration dataset emission.

Mirrors `scripts/generate_dataset.py` of the reference (run_episode :83-198, main :201-333,
feature schema `mujoco_manip/features.py:10-106`), with the episodes run side by side on the
MI355X instead of one after another:

* every slot of a `PickPlaceVecEnv` runs one episode: `plan(ACTION_REPEAT)` on device, the frame
  is built from the PRE-step observation plus the FSM's commanded target in four SE(3)
  encodings, then `step(abs_pos action)`; the staged reward components of the step land in
  `next.reward` (reference :140-196);
* an episode ends when its FSM reaches DONE (terminated / truncated are ignored, as in the
  reference loop); the slot is then re-reset with the next episode's seed and task
  (episode e: task `task_list[e % len(task_list)]`, seed `SeedSequence(seed).spawn(E)[e]`
  when `randomize_objects`, reference :267-277);
* each step's frames are gathered on device and streamed to pinned host memory (device memory
  O(envs)); finished episodes go to a streaming writer in the LeRobot v3.0 on-disk layout
  (parquet data files, `meta/info.json`, `meta/tasks.parquet`, `meta/episodes/...parquet`,
  `meta/stats.json`) plus the reference's `metadata.json` (generation config + `episode_seeds`,
  :306-319), so host memory holds only the episodes in flight.

Camera images (observation.images.overhead / .wrist, features.py:11-20, 224 x 224 RGB) come from
the batched HIP renderer (mmx_render.hip): the PRE-step images of every active
slot are gathered on device each step, encoded to PNG files on the device (mmx_png.hip) and stored the way LeRobot stores
`dtype: image` features with use_videos=False (generate_dataset.py:250-260): a parquet struct
column {bytes: PNG, path} per frame, per-channel image statistics in meta/stats.json.
LeRobot itself is not importable here, so the on-disk layout follows LeRobot v3.0's documented
format without a round-trip check against the library ("format unpinned"); the frame VALUES are
pinned against the oracle running the reference loop (tests/test_dataset.py).
"""
from __future__ import annotations

import argparse
import functools
import json
import os

import numpy as np

from . import _lib
from .constants import ACTION_REPEAT, BINS, IMAGE_SIZE, OBJECTS, OBS_SLICES, TASK_SETS
# the on-disk side (no GPU): the episode record, the LeRobot v3.0 writer, reader and shard merge
from .lerobot import (FEATURES, Episode, LeRobotWriter, PngFrames, _features_at, _merge_image_stats,  # noqa: F401
                      _png_nbytes, make_task_string, merge_shards, png_decode, png_encode, read_lerobot_v3,
                      resolve_features, write_lerobot_v3)

# generate_dataset.py:26-38 (+ the flattened keypoints :158-168)
OBS_TO_FEATURE = {
    "state": "observation.state",
    "state.ee.pos_quat_g": "observation.state.ee.pos_quat_g",
    "state.ee.pos_rot6d_g": "observation.state.ee.pos_rot6d_g",
    "state.ee.pos_quat_g_rel": "observation.state.ee.pos_quat_g_rel",
    "state.ee.pos_rot6d_g_rel": "observation.state.ee.pos_rot6d_g_rel",
    "target_bin_onehot": "observation.target_bin_onehot",
    "target_obj_onehot": "observation.target_obj_onehot",
    "target_obj_keypoints_overhead": "observation.target_obj_keypoints_overhead",
    "target_bin_keypoints_overhead": "observation.target_bin_keypoints_overhead",
    "keypoints_overhead": "observation.keypoints_overhead",
    "keypoints_wrist": "observation.keypoints_wrist",
}
ACTION_KEYS = ("action.ee.pos_quat_g", "action.ee.pos_rot6d_g", "action.ee.pos_quat_g_rel", "action.ee.pos_rot6d_g_rel")
IMAGE_KEYS = ("observation.images.overhead", "observation.images.wrist")

# pick_and_place.py:12-49 (State order = device FSM codes 0..10) and :128-149
_STATE_PHASE = ["idle", "approaching", "grasping", "grasping", "lifting", "transporting", "transporting",
                "placing", "placing", "retreating", "done"]
FSM_DONE = 10

# controller.py TARGET_ORI: the FSM's commanded hand orientation
TARGET_ORI = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])


@functools.lru_cache(maxsize=None)
def _phase_lut(obj_name: str, bin_name: str) -> list:
    """phase_description of every device FSM code for one task."""
    return [phase_description(k, obj_name, bin_name) for k in range(len(_STATE_PHASE))]


@functools.lru_cache(maxsize=None)
def phase_description(state: int, obj_name: str, bin_name: str) -> str:
    """PickAndPlaceTask.phase_description (pick_and_place.py:128-149) for a device FSM code."""
    phase = _STATE_PHASE[int(state)]
    if phase in ("idle", "done"):
        return "idle"
    if phase == "retreating":
        return "retreating to neutral position"
    o, b = obj_name.replace("obj_", ""), bin_name.replace("bin_", "")
    return {"approaching": f"approaching the {o} cube", "grasping": f"grasping the {o} cube",
            "lifting": f"lifting the {o} cube", "transporting": f"transporting the {o} cube to the {b} bin",
            "placing": f"placing the {o} cube in the {b} bin"}[phase]


# ----------------------------------------------------------------------------- action encodings
def _quat_xyzw_t(R):
    """rotmat_to_quat_xyzw (pose_utils.py:48-82) on a batch [n, 3, 3], branch for branch."""
    import torch

    r00, r11, r22 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    tr = r00 + r11 + r22
    one = torch.ones_like(tr)

    def safe_s(v):
        return 2.0 * torch.sqrt(torch.clamp(v, min=0.0) + 0.0) + (v <= 0).to(v.dtype) * 1.0  # never 0 in unused lanes

    s0 = safe_s(tr + 1.0)
    q0 = torch.stack([(R[:, 2, 1] - R[:, 1, 2]) / s0, (R[:, 0, 2] - R[:, 2, 0]) / s0, (R[:, 1, 0] - R[:, 0, 1]) / s0,
                      0.25 * s0], 1)
    s1 = safe_s(one + r00 - r11 - r22)
    q1 = torch.stack([0.25 * s1, (R[:, 0, 1] + R[:, 1, 0]) / s1, (R[:, 0, 2] + R[:, 2, 0]) / s1,
                      (R[:, 2, 1] - R[:, 1, 2]) / s1], 1)
    s2 = safe_s(one + r11 - r00 - r22)
    q2 = torch.stack([(R[:, 0, 1] + R[:, 1, 0]) / s2, 0.25 * s2, (R[:, 1, 2] + R[:, 2, 1]) / s2,
                      (R[:, 0, 2] - R[:, 2, 0]) / s2], 1)
    s3 = safe_s(one + r22 - r00 - r11)
    q3 = torch.stack([(R[:, 0, 2] + R[:, 2, 0]) / s3, (R[:, 1, 2] + R[:, 2, 1]) / s3, 0.25 * s3,
                      (R[:, 1, 0] - R[:, 0, 1]) / s3], 1)
    b0 = (tr > 0)[:, None]
    b1 = ((r00 > r11) & (r00 > r22))[:, None]
    b2 = (r11 > r22)[:, None]
    return torch.where(b0, q0, torch.where(b1, q1, torch.where(b2, q2, q3)))


_TARGET_ORI_DEV = {}


def encode_actions(target, gripper, T_init):
    """get_actions (generate_dataset.py:57-80) batched on device.

    target [n, 3], gripper [n], T_init [n, 4, 4] -> the four float32 encodings of the commanded
    SE(3) (absolute and relative to T_init), computed in float64 like the reference's numpy.
    """
    import torch

    dev = target.device
    n = target.shape[0]
    t = target.to(torch.float64)
    g = gripper.to(torch.float64)[:, None]
    Ti = T_init.to(torch.float64)
    key = str(dev)
    if key not in _TARGET_ORI_DEV:  # (a host -> device copy waits for the device: once per device)
        _TARGET_ORI_DEV[key] = torch.as_tensor(TARGET_ORI, dtype=torch.float64, device=dev)
    Rt = _TARGET_ORI_DEV[key].expand(n, 3, 3)
    # inv(T_init) @ T_target for a rigid transform: R' = Ri^T Rt, p' = Ri^T (t - pi)
    RiT = Ti[:, :3, :3].transpose(1, 2)
    Rr = RiT @ Rt
    pr = (RiT @ (t - Ti[:, :3, 3])[:, :, None])[:, :, 0]
    qa = _quat_xyzw_t(Rt)
    qr = _quat_xyzw_t(Rr)
    out = {
        "action.ee.pos_quat_g": torch.cat([t, qa, g], 1),
        "action.ee.pos_rot6d_g": torch.cat([t, Rt[:, :2, :].reshape(n, 6), g], 1),
        "action.ee.pos_quat_g_rel": torch.cat([pr, qr, g], 1),
        "action.ee.pos_rot6d_g_rel": torch.cat([pr, Rr[:, :2, :].reshape(n, 6), g], 1),
    }
    return {k: v.to(torch.float32) for k, v in out.items()}


# ----------------------------------------------------------------------------- batched collection
def resolve_tasks(task=None, tasks="all"):
    """generate_dataset.py:205-216 (same ValueErrors)."""
    if task is not None:
        pair = tuple(task)
        if len(pair) != 2:
            raise ValueError(f"task must be [obj, bin], got {pair}")
        return [pair]
    if tasks in TASK_SETS:
        return TASK_SETS[tasks]
    raise ValueError(f"Unknown task set '{tasks}'. Choose from: {list(TASK_SETS.keys())}")


def episode_seeds(seed: int, num_episodes: int) -> list[int]:
    """generate_dataset.py:263-268: SeedSequence(seed).spawn(E)[e].generate_state(1)[0]."""
    return [_lib.episode_seed(seed, e) for e in range(num_episodes)]


def rank_episodes(num_episodes: int, rank: int = 0, world_size: int = 1) -> list[int]:
    """Global episode indices a rank generates when the dataset is sharded over `world_size`
    processes (one per GPU): e = rank (mod world_size).  An episode keeps its global
    seed and task (generate_dataset.py:263-277), so the frames do not depend on the rank count."""
    if not (0 <= rank < world_size):
        raise ValueError(f"bad shard: rank {rank} of {world_size}")
    return list(range(rank, int(num_episodes), world_size))


def shard_dir(path: str, rank: int, world_size: int) -> str:
    """Where rank `rank` of `world_size` writes its LeRobot shard inside the dataset directory."""
    return os.path.join(path, f"shard-{rank:03d}-of-{world_size:03d}")


class _PinnedRing:
    """Pinned host staging for the per-step frame copies: device tensors are copied with
    non_blocking=True on a side stream that waits for the producing stream, an event marks
    completion, and at most `depth` copies are in flight (older ones are waited first)."""

    def __init__(self, dev, depth=4):
        import torch

        self.torch = torch
        self.stream = torch.cuda.Stream(device=dev)
        self.depth = depth
        self.pending = []  # (event, host dict, payload)

    def push(self, tensors: dict, payload):
        torch = self.torch
        self.stream.wait_stream(torch.cuda.current_stream(self.stream.device))
        host = {}
        with torch.cuda.stream(self.stream):
            for k, v in tensors.items():
                h = torch.empty(v.shape, dtype=v.dtype, pin_memory=True)
                h.copy_(v, non_blocking=True)
                v.record_stream(self.stream)
                host[k] = h
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.pending.append((ev, host, payload))

    def ready(self, drain=False):
        """Completed copies, oldest first, as (host dict of numpy arrays, payload); waits for the
        oldest ones beyond `depth`, and with `drain` for all of them."""
        out = []
        while self.pending and (drain or self.pending[0][0].query() or len(self.pending) > self.depth):
            ev, host, payload = self.pending.pop(0)
            ev.synchronize()
            out.append(({k: v.numpy() for k, v in host.items()}, payload))
        return out

    def drain(self):
        return self.ready(drain=True)


# [min, max, sum, sum of squares] of the uint8 values -> the same of the values scaled to [0, 1]
_STAT_SCALE = (1.0 / 255.0, 1.0 / 255.0, 1.0 / 255.0, 1.0 / (255.0 * 255.0))
_STAT_SCALE_DEV = {}


def _frame_image_stats_device(sim, imgs):
    """Per-frame channel statistics of uint8 images [k, H, W, 3] by the HIP kernel mmx_image_stats
    (one pass over the frames, exact integers) -> float64 [k, 4, 3], the values of
    _frame_image_stats bit for bit (the same integers scaled by the same constants)."""
    import torch

    st = sim.image_stats(imgs).to(torch.float64)
    scale = _STAT_SCALE_DEV.get(st.device)
    if scale is None:  # cached per device: a host-to-device copy per step would wait for the queue
        scale = _STAT_SCALE_DEV[st.device] = torch.tensor(_STAT_SCALE, dtype=torch.float64, device=st.device)[None, :, None]
    return st * scale


def _frame_image_stats(imgs, chunk=None):
    """Torch form of _frame_image_stats_device (the reference for its test; the dataset loop uses
    the kernel): min, max, sum and sum of squares of the pixel values scaled to [0, 1] -> float64
    [k, 4, 3].  Min / max on the uint8 values, sums exact in integers (int32 values, int64 sums) and
    scaled at the end, in chunks of `chunk` images (default: 256 MB of int32 values)."""
    import torch

    k = imgs.shape[0]
    if chunk is None:
        chunk = max(1, (1 << 26) // max(1, imgs[0].numel()))
    x = imgs.reshape(k, -1, 3)
    out = torch.empty((k, 4, 3), dtype=torch.float64, device=imgs.device)
    out[:, 0] = x.amin(1).to(torch.float64) * (1.0 / 255.0)
    out[:, 1] = x.amax(1).to(torch.float64) * (1.0 / 255.0)
    for a in range(0, k, chunk):
        xi = x[a:a + chunk].to(torch.int32)
        out[a:a + chunk, 2] = xi.sum(1, dtype=torch.int64).to(torch.float64) * (1.0 / 255.0)
        out[a:a + chunk, 3] = (xi * xi).sum(1, dtype=torch.int64).to(torch.float64) * (1.0 / (255.0 * 255.0))
    return out


class _EpisodeAssembler:
    """Host side of collect_episodes (numpy and the host helper mmx_copy_ranges: no torch, no device):
    puts the per-step copies back together into episodes and hands them to `sink(episode)` in index
    order, or, without a sink, collects them in `episodes`.  step(host, png) takes one step as the
    ring yields it: `_q_slot` (slot -> local episode, -1 = none), `_q_fin` (the episode that ended in
    the slot), `_fsm`, the numeric features [N, ...], per camera `<key>/ends` (the N files' running
    end offsets) and `<key>/stats`; `png[key]`: the step's complete packed files.

    A slot's running episode gets one row per step in the slot's buffers, written for all of the
    step's slots at once; its rows are copied out when it finishes, before the slot's next episode
    writes there.  Its PNG files grow in one uint8 buffer per camera: each step's files are appended
    straight out of the pinned copy by one C call per camera (no Python object per frame, the GIL
    released), and the finished episode takes the buffer with it as PngFrames (no further copy)."""

    def __init__(self, eps, num_slots, feature_keys, image_size, copy_ranges, sink=None):
        N, cams = int(num_slots), [f for f in IMAGE_KEYS if f in feature_keys]
        self.eps, self.N, self.feature_keys, self.sink = eps, N, feature_keys, sink
        self.npx, self.copy_ranges = image_size * image_size, copy_ranges
        self.episodes = [] if sink is None else None
        self.emitted = 0  # episodes [0, emitted) have left
        self.done_eps = set()  # finished, awaiting in-order emission
        self.started = self.over = False  # over: a step with no episode in any slot after the first with one
        self.ep_slot = np.full(len(eps), -1, np.int64)  # the slot an episode ran in
        self.bufs = {}  # host key -> [N, cap, ...]
        self.cap = 64
        self.tpos = np.zeros(N, np.int64)  # rows of the slot's current episode so far
        self.buf_ep = np.full(N, -1, np.int64)  # the episode whose rows the slot holds
        self.png_buf = {f: [None] * N for f in cams}  # camera -> slot -> buffer
        self.png_addr = {f: np.zeros(N, np.uint64) for f in cams}  # the buffers' addresses
        self.png_fill = {f: np.zeros(N, np.int64) for f in cams}  # bytes used
        self.png_cap = {f: np.zeros(N, np.int64) for f in cams}  # bytes allocated
        # first buffer size of an episode: 1.25 x the largest finished episode so far; before any has
        # finished, 160 frames of the first step's mean file size (grown by doubling when exceeded)
        self.png_guess = {f: 0 for f in cams}
        self.png_regrown = 0  # buffers reallocated with their bytes so far carried over

    def step(self, host, png):
        fin = host["_q_fin"]
        for e in fin[fin >= 0].tolist():  # ended before this step: every row of theirs is absorbed
            self._finish(e)
        slot = host["_q_slot"]
        act = np.nonzero(slot >= 0)[0]
        if len(act):
            self.started = True
            self._absorb(host, act, slot[act].astype(np.int64), png)
        else:
            self.over = self.over or self.started
        self._emit_ready()

    def open_ids(self):
        """Global indices of the episodes not finished yet."""
        return [int(self.eps[e].index) for e in range(self.emitted, len(self.eps)) if e not in self.done_eps]

    def close_open(self):
        """Finish the episodes still open with the rows they have, and emit everything."""
        for e in range(self.emitted, len(self.eps)):
            if e not in self.done_eps:
                self._finish(e)
        self._emit_ready()

    def _png_alloc(self, f, s, cap, keep=0):
        buf = np.empty(int(cap), np.uint8)
        if keep:
            buf[:keep] = self.png_buf[f][s][:keep]
            self.png_regrown += 1
        self.png_buf[f][s] = buf
        self.png_addr[f][s] = buf.ctypes.data
        self.png_cap[f][s] = len(buf)

    def _absorb(self, host, slots, ep_ids, png):
        N, tpos, buf_ep, bufs = self.N, self.tpos, self.buf_ep, self.bufs
        self.ep_slot[ep_ids] = slots
        new = buf_ep[slots] != ep_ids
        if new.any():
            ns = slots[new]
            tpos[ns] = 0
            buf_ep[ns] = ep_ids[new]
            for f in self.png_buf:
                self.png_fill[f][ns] = 0
                for s in ns.tolist():
                    self._png_alloc(f, s, self.png_guess[f] or (1 << 16))
        for f, data in png.items():  # append the step's files to their episodes' buffers
            fill, pcap = self.png_fill[f], self.png_cap[f]
            ends = host[f + "/ends"]
            if self.png_guess[f] == 0:
                guess = self.png_guess[f] = 160 * max(1, int(ends[-1]) // max(1, len(ends)))
                for s in np.nonzero(pcap[slots] < guess)[0].tolist():
                    if fill[slots[s]] == 0:
                        self._png_alloc(f, int(slots[s]), guess)
            starts = np.zeros_like(ends)
            starts[1:] = ends[:-1]
            plen = host[f + "/plen"] = (ends - starts).astype(np.int64)  # a row like the features': file sizes
            lens = plen[slots]
            need = fill[slots] + lens
            for k in np.nonzero(need > pcap[slots])[0].tolist():  # (rare) grow
                s = int(slots[k])
                self._png_alloc(f, s, max(2 * int(need[k]), self.png_guess[f]), keep=int(fill[s]))
            src = (data.ctypes.data + starts[slots].astype(np.uint64)).astype(np.uint64)
            dst = self.png_addr[f][slots] + fill[slots].astype(np.uint64)
            if self.copy_ranges(len(slots), src.ctypes.data, dst.ctypes.data, lens.ctypes.data) != int(lens.sum()):
                raise RuntimeError("mmx_copy_ranges failed")
            fill[slots] = need
        t = tpos[slots]
        if int(t.max()) >= self.cap:
            self.cap *= 2
            for k, v in bufs.items():
                g = np.empty((N, self.cap) + v.shape[2:], v.dtype)
                g[:, :v.shape[1]] = v
                bufs[k] = g
        cap = self.cap
        flat = slots * cap + t  # row (slot, t) of a [N, cap, ...] buffer as one flat index: numpy's
        for k, v in host.items():  # two-array fancy index is ~8x slower for the same scatter
            if k.endswith("/png") or k.endswith("/ends") or k.startswith("_q"):
                continue
            if k not in bufs:
                bufs[k] = np.empty((N, cap) + v.shape[1:], v.dtype)
            b = bufs[k]
            b.reshape((N * cap,) + b.shape[2:])[flat] = v[slots]
        tpos[slots] = t + 1

    def _finish(self, e):
        """Copy episode e's rows out of its slot's buffers (it has ended: no row of it is still in
        flight, and the slot's next episode has not written yet)."""
        ep, bufs = self.eps[e], self.bufs
        s = int(self.ep_slot[e])
        L = int(self.tpos[s]) if s >= 0 and self.buf_ep[s] == e else 0
        ep.length = L
        ep.image_stats = {}
        for k in self.feature_keys:
            if k in IMAGE_KEYS:
                if L:
                    offs = np.zeros(L + 1, np.int64)
                    np.cumsum(bufs[k + "/plen"][s, :L], out=offs[1:])
                    if offs[-1] != self.png_fill[k][s]:
                        raise RuntimeError(f"episode {ep.index}: PNG bytes {self.png_fill[k][s]} != frames {offs[-1]}")
                    ep.frames[k] = PngFrames(self.png_buf[k][s][:int(offs[-1])], offs)
                    self.png_buf[k][s] = None
                    self.png_guess[k] = max(self.png_guess[k], int(offs[-1]) * 5 // 4)
                else:
                    ep.frames[k] = []
                ep.image_stats[k] = _merge_image_stats(bufs[k + "/stats"][s, :L], self.npx) if L else None
            elif k == "observation.phase_description":
                lut = _phase_lut(ep.obj, ep.bin)
                ep.frames[k] = [lut[v] for v in bufs["_fsm"][s, :L].tolist()] if L else []
            elif L and k in bufs:
                ep.frames[k] = bufs[k][s, :L].astype(np.float32)
        if L:
            self.buf_ep[s] = -1
        self.done_eps.add(e)

    def _emit_ready(self):
        while self.emitted in self.done_eps:
            e = self.emitted
            self.done_eps.remove(e)
            if self.sink is not None:
                self.sink(self.eps[e])
                self.eps[e] = None  # the sink owns it now: host memory stays bounded by the episodes in flight
            else:
                self.episodes.append(self.eps[e])
            self.emitted += 1


def _step_frame(env, action, feature_keys, png_est):
    """One step's device tensors for the ring, from the env BEFORE its step -> (frame, payload);
    payload: camera -> the whole packed PNG buffer, of which the frame carries a prefix of
    `png_est` bytes (first seen: a quarter of the buffer)."""
    frame, payload = {}, {}
    obs_pre = env._obs.clone()  # PRE-step obs (from the reset or the previous step)
    for k, f in OBS_TO_FEATURE.items():
        if f in feature_keys:
            a, b, _ = OBS_SLICES[k]
            frame[f] = obs_pre[:, a:b]
    for cam, f in enumerate(IMAGE_KEYS):  # PRE-step images (rendered after the reset / previous step)
        if f not in feature_keys:
            continue
        imgs = env._images[:, cam]
        packed, ends = env.sim.png_encode_device(imgs)
        if f not in png_est:
            png_est[f] = packed.numel() // 4
        frame[f + "/png"] = packed[:min(png_est[f], packed.numel())]
        frame[f + "/ends"] = ends
        frame[f + "/stats"] = _frame_image_stats_device(env.sim, imgs)
        payload[f] = packed
    act_keys = [k for k in ACTION_KEYS if k in feature_keys]
    if act_keys:
        enc = encode_actions(action[:, :3], action[:, 3], env.initial_ee_se3)
        for k in act_keys:
            frame[k] = enc[k]
    frame["_fsm"] = env._epi[:, _lib.EPI["fsm_state"]].clone()
    return frame, payload


def collect_episodes(num_episodes: int, task_list, feature_keys, *, reward_type="staged", randomize_objects=False,
                     seed=0, spawn_x_range=(-0.20, 0.20), spawn_y_range=(0.30, 0.45), num_envs=1024, device=0,
                     max_gym_steps=5000, on_step=None, sink=None, image_size=IMAGE_SIZE, episode_ids=None,
                     render_effects=()):
    """Run `num_episodes` reference run_episode loops (generate_dataset.py:83-198) side by side,
    or, with `episode_ids`, only those episodes of the `num_episodes`-episode job (a rank's shard,
    rank_episodes): each keeps its global index, seed and task.

    Streaming with no host synchronisation per step: the slot -> episode assignment runs on the
    device (mmx_queue_advance), each step's frames of every slot (plus the assignment) are copied
    to pinned host memory on a side stream, and the host splits them into their episodes a few
    steps later, as the copies complete.  Camera frames are
    encoded to PNG files on the device (mmx_png_encode; LeRobot embeds image features as PNG,
    generate_dataset.py:250-260) with their per-channel statistics, so only the compressed files
    cross PCIe and the host does no image work.  Device memory is O(envs): no frame stays on the
    device after its copy; the packed PNG buffers of the steps in flight (ring depth 4 + 1, room for
    n bounds each) dominate it: 13 GB at 128^2 and 32 GB at 224^2 for 8192 envs.  A finished episode (FSM DONE) is handed to `sink(episode)` in
    episode-index order, so the host holds only the episodes in flight; without a sink the episodes
    are returned as a list.  on_step(slots, episode_ids, env), when given, sees the env before each
    batched step (a diagnostic hook: it costs a host synchronisation per step).  Returns (episodes or
    None, seeds).
    """
    import torch

    from .vec_env import PickPlaceVecEnv

    seeds = episode_seeds(seed, int(num_episodes)) if randomize_objects else None
    ids = list(range(int(num_episodes))) if episode_ids is None else [int(g) for g in episode_ids]
    if any(not 0 <= g < int(num_episodes) for g in ids):
        raise ValueError(f"episode ids must lie in [0, {num_episodes})")
    E = len(ids)
    if E == 0:
        return ([] if sink is None else None), seeds
    N = max(1, min(int(num_envs), E))
    use_images = bool(set(feature_keys) & set(IMAGE_KEYS))
    env = PickPlaceVecEnv(N, tasks=[tuple(t) for t in task_list], action_mode="abs_pos", reward_type=reward_type,
                          randomize_objects=randomize_objects, spawn_x_range=tuple(spawn_x_range),
                          spawn_y_range=tuple(spawn_y_range), autoreset=False, device=device,
                          image_size=image_size if use_images else 0,
                          render_effects=tuple(render_effects) if use_images else ())
    need_reward = "next.reward" in feature_keys and reward_type == "staged"

    # local position e <-> global episode ids[e]: slots and rows are indexed locally.  The slot ->
    # episode assignment runs on the device (mmx_queue_advance): a slot whose episode's FSM reached
    # DONE takes the next episode and is reset with its seed and task, in ascending slot order, with
    # no host synchronisation; the host learns the assignment from the per-step copies.
    eps = [Episode(g, *task_list[g % len(task_list)], seeds[g] if seeds else None) for g in ids]
    env.sim.queue_init([(OBJECTS.index(ep.obj) << 4) | BINS.index(ep.bin) for ep in eps],
                       [ep.seed for ep in eps] if seeds else None)
    asm = _EpisodeAssembler(eps, N, feature_keys, image_size, env.sim.L.mmx_copy_ranges, sink)
    ring = _PinnedRing(env.device)
    slot_dev = torch.empty(N, dtype=torch.int32, device=env.device)
    fin_dev = torch.empty(N, dtype=torch.int32, device=env.device)
    png_est = {}  # camera feature -> bytes copied per step: 1.25 x the largest packed size seen + 1 MB
    png_max = {}

    def assemble(items):
        for host, payload in items:
            png = {}
            for f, packed in payload.items():  # the step's packed PNG files (copied: a prefix)
                total = int(host[f + "/ends"][-1])
                data = host[f + "/png"]
                if total > len(data):  # more than the estimate: fetch the rest (rare)
                    data = np.concatenate([data, packed[len(data):total].cpu().numpy()])
                png_max[f] = max(png_max.get(f, 0), total)
                png_est[f] = (png_max[f] * 5) // 4 + (1 << 20)
                png[f] = data
            asm.step(host, png)

    step_no = 0
    while not asm.over:
        # the host learns that the last episode ended from copies up to ring.depth steps behind the
        # device: allow that lag past the limit before calling the run unfinished
        if step_no >= max_gym_steps + ring.depth:
            assemble(ring.drain())
            if asm.over:
                break
            still = asm.open_ids()
            raise RuntimeError(f"episodes did not finish within {max_gym_steps} gym steps: {len(still)} still "
                               f"open, e.g. {still[:16]}")
        env.sim.queue_advance(slot_dev.data_ptr(), fin_dev.data_ptr())  # resets the slots it assigns
        action = env.expert_plan(ACTION_REPEAT)  # fsm.plan(16) -> (target, gripper) for every slot
        frame, payload = _step_frame(env, action, feature_keys, png_est)
        frame["_q_slot"], frame["_q_fin"] = slot_dev.clone(), fin_dev.clone()
        if on_step is not None:  # diagnostic hook: reads the assignment back (a host sync per step)
            sl = slot_dev.cpu().numpy()
            act_slots = np.nonzero(sl >= 0)[0]
            on_step(act_slots, np.asarray(ids, np.int64)[sl[act_slots]], env)
        env.sim.step(action.data_ptr(), action.shape[1])
        if need_reward:
            frame["next.reward"] = env._rc.clone()
        ring.push(frame, payload)
        assemble(ring.ready())
        step_no += 1
    assemble(ring.drain())
    asm.close_open()  # episodes still open when the loop ended (none, unless max_gym_steps cut it)
    torch.cuda.synchronize(env.device)
    env.close()
    return asm.episodes, seeds


# ----------------------------------------------------------------------------- entry point
def generate(repo_id, num_episodes=100, root="./datasets", task=None, tasks="all", reward_type="staged",
             randomize_objects=False, seed=0, spawn_x_range=(-0.20, 0.20), spawn_y_range=(0.30, 0.45),
             features=None, num_envs=1024, device=0, image_size=IMAGE_SIZE, rank=0, world_size=1,
             render_effects=()):
    """generate_dataset.main (generate_dataset.py:201-333) with the episodes batched on the GPU and
    streamed to the LeRobot writer as they finish.

    Sharded (world_size > 1, one process per GPU): rank r generates the episodes
    e = r (mod world_size) with their global seeds and tasks and writes them as a LeRobot dataset
    of its own in `<root>/<repo_id>/shard-RRR-of-WWW` (local episode indices 0..n-1, the global
    ones in its metadata.json under "shard"); merge_shards then writes the dataset a single
    process would have written.  render_effects: the opt-in camera effects of the frames
    ("shadows", "translucent_bins"; PickPlaceVecEnv), recorded in the stored config when not empty.
    Returns (path written, info)."""
    render_effects = tuple(render_effects or ())
    _lib.render_effect_flags(render_effects)  # names checked before anything is written
    if not repo_id:
        raise ValueError("repo_id is required (e.g. repo_id=user/pick-place)")
    task_list = resolve_tasks(task, tasks)
    feats = _features_at(resolve_features(features, reward_type), image_size)
    path = os.path.join(root, repo_id)
    ids = rank_episodes(num_episodes, rank, world_size)
    out = path if world_size == 1 else shard_dir(path, rank, world_size)
    writer = LeRobotWriter(out, repo_id, feats, threaded=True, keep_image_sums=world_size > 1)
    local = []

    def sink(ep):  # shard-local episode numbering (a LeRobot dataset counts from 0)
        local.append(ep.index)
        ep.index = len(local) - 1
        writer.add_episode(ep)

    _, seeds = collect_episodes(num_episodes, task_list, set(feats), reward_type=reward_type,
                                randomize_objects=randomize_objects, seed=seed, spawn_x_range=spawn_x_range,
                                spawn_y_range=spawn_y_range, num_envs=num_envs, device=device, sink=sink,
                                image_size=image_size, episode_ids=ids, render_effects=render_effects)
    cfg = {"repo_id": repo_id, "num_episodes": int(num_episodes), "root": root,
           "task": list(task) if task is not None else None, "tasks": tasks, "reward_type": reward_type,
           "randomize_objects": bool(randomize_objects), "seed": int(seed), "spawn_x_range": list(spawn_x_range),
           "spawn_y_range": list(spawn_y_range), "push_to_hub": False, "private": True,
           "features": list(features) if features is not None else None}
    if image_size != IMAGE_SIZE:
        cfg["image_size"] = int(image_size)
    if render_effects:
        cfg["render_effects"] = list(render_effects)
    if seeds is not None:
        cfg["episode_seeds"] = [int(s) for s in seeds]
    md = cfg if world_size == 1 else dict(cfg, shard={"rank": int(rank), "world_size": int(world_size),
                                                      "global_episode_index": local})
    info = writer.close(extra_info={"generation_config": md})
    with open(os.path.join(out, "metadata.json"), "w") as f:
        json.dump(md, f, indent=2)
    return out, info



def main(argv=None):
    ap = argparse.ArgumentParser(description="Generate a LeRobot v3.0 dataset from batched expert FSM episodes")
    ap.add_argument("--repo-id", required=True)
    ap.add_argument("--num-episodes", type=int, default=100)
    ap.add_argument("--root", default="./datasets")
    ap.add_argument("--task", nargs=2, default=None, metavar=("OBJ", "BIN"))
    ap.add_argument("--tasks", default="all")
    ap.add_argument("--reward-type", default="staged")
    ap.add_argument("--randomize-objects", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--spawn-x-range", type=float, nargs=2, default=(-0.20, 0.20))
    ap.add_argument("--spawn-y-range", type=float, nargs=2, default=(0.30, 0.45))
    ap.add_argument("--features", nargs="*", default=None)
    ap.add_argument("--num-envs", type=int, default=1024, help="parallel envs per GPU")
    ap.add_argument("--image-size", type=int, default=IMAGE_SIZE)
    ap.add_argument("--render-effects", nargs="*", default=(), choices=("shadows", "translucent_bins"),
                    help="opt-in camera effects: cast shadows, translucent bins (default: neither)")
    ap.add_argument("--no-merge", action="store_true", help="sharded run: keep the per-rank shards only")
    ap.add_argument("--dist-backend", default=None, help="sharded run: collective backend (default nccl = RCCL)")
    a = ap.parse_args(argv)
    # one process per GPU under torchrun (RANK / LOCAL_RANK / WORLD_SIZE): each rank writes its
    # shard, a gather of the per-rank summaries (the only collective) tells rank 0 they are done
    rank, local_rank, world = (int(os.environ.get(k, d)) for k, d in (("RANK", 0), ("LOCAL_RANK", 0), ("WORLD_SIZE", 1)))
    import time

    t0 = time.perf_counter()
    path, info = generate(a.repo_id, a.num_episodes, a.root, a.task, a.tasks, a.reward_type, a.randomize_objects,
                          a.seed, a.spawn_x_range, a.spawn_y_range, a.features, a.num_envs, device=local_rank,
                          image_size=a.image_size, rank=rank, world_size=world, render_effects=tuple(a.render_effects))
    summary = [float(info["total_episodes"]), float(info["total_frames"]), time.perf_counter() - t0]
    if world > 1:
        import torch
        import torch.distributed as dist

        backend = a.dist_backend or ("nccl" if torch.cuda.is_available() else "gloo")
        dist.init_process_group(backend)
        dev = torch.device("cuda", local_rank) if backend == "nccl" else torch.device("cpu")
        mine = torch.tensor(summary, dtype=torch.float64, device=dev)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        dist.destroy_process_group()
        if rank != 0:
            return
        per_rank = [t.cpu().tolist() for t in every]
        print(json.dumps({"shards": [{"rank": r, "episodes": int(e), "frames": int(f), "seconds": round(s, 3)}
                                     for r, (e, f, s) in enumerate(per_rank)]}))
        if a.no_merge:
            return
        info = merge_shards(os.path.join(a.root, a.repo_id))
        path = os.path.join(a.root, a.repo_id)
    print(f"Dataset saved to {path}: {info['total_episodes']} episodes, {info['total_frames']} frames")


if __name__ == "__main__":
    main()
