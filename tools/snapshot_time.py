"""Snapshot / restore timing (experiment infrastructure): what mmx_snapshot and mmx_restore cost on the
C3 shape (4096 envs, all tasks, randomised, staged reward, no cameras) next to the host round trip they
replace and to one env step, all in one run.

A fresh env, the seeded reset, 40 env steps of the on-device expert untimed (the envs are then spread over
the approach and grasp phases), then five rounds; in a round each line is warmed once and then timed:
  snapshot            mmx_snapshot of all envs into a caller-owned blob
  restore_identity    mmx_restore, env i <- record i (src_dev = NULL)
  restore_broadcast   mmx_restore, every env <- record 0 (the planner's branch)
  step                mmx_step with the expert's action (the order kernel and the step kernel)
  host_round_trip     mmx_get_state + mmx_set_state of qpos, qvel, ctrl, qacc_warmstart
The device lines are timed with a pair of events on the sim's stream around REPS back-to-back calls (the
figure is the time per call as the stream sees it, launch gaps included; a lone launch of a kernel this
small mostly measures the event pair); the host round trip is synchronous and timed on the host clock.
The restores put back the state the snapshot was taken from, so every round steps the same envs.

  python tools/snapshot_time.py [--envs 4096] [--out profiles/r10_snapshot.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from mujoco_manip_amd import _lib  # noqa: E402

ROUNDS, ADVANCE, SEED = 5, 40, 42
REPS = {"snapshot": 200, "restore_identity": 200, "restore_broadcast": 200, "step": 10, "host_round_trip": 5}


def make_env(n):
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(n, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          autoreset=True, image_size=0)
    env.reset(seed=[_lib.episode_seed(SEED, i) for i in range(n)])
    return env


def event_timed(env, f, reps) -> float:
    """Seconds per call of `reps` back-to-back calls of f, between two events on the sim's stream."""
    f()
    env.sim.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def host_timed(env, f, reps) -> float:
    f()
    env.sim.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        f()
    env.sim.synchronize()
    return (time.perf_counter() - t) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r10_snapshot.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("snapshot_time.py needs the MI355X: there is nothing to time without it")
    n = a.envs
    env = make_env(n)
    sim = env.sim
    env.rollout_expert(ADVANCE)
    action = env.expert_plan(16)
    snap = env.snapshot()
    blob, nb = snap.data, sim.snapshot_bytes
    zeros = torch.zeros(n, dtype=torch.int32, device=env.device)
    env.synchronize()
    qpos0 = env.qpos.cpu().numpy().copy()

    def round_trip():
        sim.set_state(*sim.get_state())

    lines = {
        "snapshot": (event_timed, lambda: sim.snapshot(blob.data_ptr())),
        "restore_identity": (event_timed, lambda: sim.restore(blob.data_ptr(), n)),
        "restore_broadcast": (event_timed, lambda: sim.restore(blob.data_ptr(), n, zeros.data_ptr())),
        "step": (event_timed, lambda: sim.step(action.data_ptr(), 4)),
        "host_round_trip": (host_timed, round_trip),
    }
    secs = {k: [] for k in lines}
    for _ in range(ROUNDS):
        for name, (timer, f) in lines.items():
            sim.restore(blob.data_ptr(), n)  # every line of every round starts from the snapshot's state
            secs[name].append(timer(env, f, REPS[name]))
    sim.restore(blob.data_ptr(), n)
    env.synchronize()
    assert np.array_equal(env.qpos.cpu().numpy(), qpos0), "the identity restore did not put the snapshot's state back"
    env.close()

    res = {"envs": n, "record_bytes": nb, "rounds": ROUNDS, "advance_steps": ADVANCE, "calls_per_timing": REPS,
           "unit": "microseconds per call", "lines": {}, "fraction_of_step": {}}
    for name, v in secs.items():
        us = [1e6 * s for s in v]
        res["lines"][name] = {"min": min(us), "median": float(np.median(us)), "max": max(us), "rounds": us}
    step = res["lines"]["step"]["median"]
    for name in lines:
        if name != "step":
            res["fraction_of_step"][name] = res["lines"][name]["median"] / step
    # bytes a call moves (read + written) over its time
    for name in ("snapshot", "restore_identity", "restore_broadcast"):
        res["lines"][name]["GB_per_s"] = 2 * n * nb / (res["lines"][name]["median"] * 1e-6) / 1e9
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"envs": n, "record_bytes": nb, "median_us": {k: round(v["median"], 2) for k, v in res["lines"].items()},
                      "fraction_of_step": {k: round(v, 5) for k, v in res["fraction_of_step"].items()}}))


if __name__ == "__main__":
    main()
