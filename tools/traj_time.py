"""Action-sequence rollout timing (experiment infrastructure): what the fused rollout and its per-step
record cost against the loops they replace, on the C3 shape (4096 envs, all tasks, randomised, staged
reward, no cameras).

The actions are the on-device expert's own, recorded first with mmx_rollout_expert_record over the whole
schedule, so the replayed steps see the real phase mix.  A measurement is one line in one round: a fresh
env, the seeded reset, 120 * round env steps untimed to move through the episode, an untimed window of
each length, then a timed window of T = 20 and one of T = 100 env steps, each from its first call to the
stream's completion.  Five rounds; within a round the lines run one after another, so drift hits all of
them alike.  One sim is alive at a time: with every line's sim alive in one process all but one of them
ran 40 % slow (probably their rollout lanes doubling up on the process's hardware queues), and one
process per line was as slow and noisier.
  a  T x Sim.step on the baseline library (--baseline-lib, e.g. the parent commit's build, bound to the
     line's sims with lib=; in a child process, as every figure under profiles/ was measured)
  b  T x Sim.step on this library
  c  mmx_rollout_actions with the full record (arrays allocated outside the timing)
  d  mmx_rollout_actions without a record
  e  mmx_rollout_expert
  f  mmx_rollout_expert_record with the full record

  python tools/traj_time.py [--baseline-lib PATH] [--envs 4096] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from mujoco_manip_amd import _lib  # noqa: E402

ROUNDS, ADVANCE, WARMUP, WINDOWS = 5, 120, (20, 100), (20, 100)  # per round: untimed steps, untimed / timed windows
SEED = 42


def make_env(n, lib=None):
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(n, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          autoreset=True, image_size=0, lib=lib)
    env.reset(seed=[_lib.episode_seed(SEED, i) for i in range(n)])
    return env


def timed(env, f) -> float:
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    env.sim.synchronize()
    return time.perf_counter() - t


def loop_window(env, acts, off, T):
    for k in range(off, off + T):
        env.sim.step(acts[k].data_ptr(), 4)


def full_record(env, T):
    arrays = {k: torch.empty((T, env.num_envs, w), dtype=getattr(torch, t), device=env.device)
              for k, (w, t) in _lib.TRAJ_FIELDS.items()}
    rec = _lib.MMXTrajectory()
    for k, v in arrays.items():
        setattr(rec, k, v.data_ptr())
    return rec, arrays


def run_round(line, r, acts, n, lib=None):
    """One measurement of `line` on the build `lib` of the library: ({T: seconds}, digest of the final qpos)."""
    env = make_env(n, lib)
    sim, off = env.sim, r * ADVANCE
    recs = {T: full_record(env, T) for T in set(WINDOWS)} if line in "cf" else {}

    def window(off, T, rec):
        if line in "ab":
            loop_window(env, acts, off, T)
        elif line in "cd":
            sim.rollout_actions(acts[off].data_ptr(), 4, T, rec)
        else:
            sim.rollout_expert(T, rec)

    if off:
        window(0, off, None)
    secs = {}
    for w, T in enumerate(WARMUP + WINDOWS):
        t = timed(env, lambda: window(off, T, recs[T][0] if recs else None))
        if w >= len(WARMUP):
            secs[T] = t
        off += T
    digest = hashlib.sha256(env.qpos.cpu().numpy().tobytes()).hexdigest()
    env.close()
    return secs, digest


def serve(lib, actions_file, n):
    """Line a on a library of another commit (_lib.load binds the calls it has; only create / reset / step /
    synchronize are used): serves round numbers on stdin with run_round's result."""
    acts = torch.as_tensor(np.load(actions_file), device="cuda")
    print("ready", flush=True)
    for req in sys.stdin:
        secs, digest = run_round("a", int(req), acts, n, lib)
        print(json.dumps([secs, digest]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--baseline-lib", default=None, help="library of the baseline commit for line a")
    ap.add_argument("--out", default=None, help="file for the full result (the summary line is printed either way)")
    ap.add_argument("--serve", nargs=2, metavar=("LIB", "ACTIONS"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.serve:
        return serve(a.serve[0], a.serve[1], a.envs)
    n, total = a.envs, (ROUNDS - 1) * ADVANCE + sum(WARMUP) + sum(WINDOWS)

    # the expert's actions over the whole schedule
    env = make_env(n)
    acts = env.rollout(n_steps=total, record=("target",))["target"]
    env.synchronize()
    env.close()
    lines, child = ["b", "c", "d", "e", "f"], None
    if a.baseline_lib:
        fd, actions_file = tempfile.mkstemp(suffix=".npy")  # (47 MB: not among the outputs)
        os.close(fd)
        np.save(actions_file, acts.cpu().numpy())
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--envs", str(n), "--serve",
                                  os.path.abspath(a.baseline_lib), actions_file],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert child.stdout.readline().strip() == "ready", "baseline child failed to start"
        os.unlink(actions_file)
        lines.insert(0, "a")
    rates = {ln: {T: [] for T in WINDOWS} for ln in lines}
    for r in range(ROUNDS):
        final = {}
        for ln in lines:
            if ln == "a":
                child.stdin.write(f"{r}\n")
                child.stdin.flush()
                secs, final[ln] = json.loads(child.stdout.readline())
                secs = {int(T): t for T, t in secs.items()}
            else:
                secs, final[ln] = run_round(ln, r, acts, n)
            for T in WINDOWS:
                rates[ln][T].append(n * T / secs[T])
        # the host-action lines followed one trajectory, the expert lines another
        assert len({final[ln] for ln in lines if ln in "abcd"}) == 1, f"host-action lines ended in different states: {final}"
        assert final["e"] == final["f"], final
    if child:
        child.stdin.close()
        child.wait(timeout=60)

    res = {"envs": n, "rounds": ROUNDS, "advance_steps_per_round": ADVANCE, "warmup_windows": list(WARMUP),
           "windows": list(WINDOWS), "unit": "env steps/s", "baseline_lib": a.baseline_lib, "lines": {}, "ratios": {}}
    for ln in lines:
        res["lines"][ln] = {f"T{T}": {"min": min(v), "median": float(np.median(v)), "max": max(v), "windows": v}
                            for T, v in sorted(rates[ln].items())}
    # ratios per round (the rounds differ in their stage of the episode; within a round both lines step the
    # same states): median and range over the rounds
    pairs = [("c", "a"), ("b", "a"), ("c", "b"), ("d", "b"), ("c", "d"), ("f", "e")]
    for T in sorted(set(WINDOWS)):
        res["ratios"][f"T{T}"] = {}
        for x, y in pairs:
            if x in rates and y in rates:
                q = [p / r for p, r in zip(rates[x][T], rates[y][T])]
                res["ratios"][f"T{T}"][f"{x}_over_{y}"] = {"min": min(q), "median": float(np.median(q)), "max": max(q)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"ratios": {T: {k: [round(v[m], 3) for m in ("min", "median", "max")] for k, v in d.items()}
                                 for T, d in res["ratios"].items()},
                      "median": {ln: {k: round(v["median"]) for k, v in d.items()} for ln, d in res["lines"].items()}}))


if __name__ == "__main__":
    main()
