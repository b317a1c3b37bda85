"""What a control step of the MPPI planner costs (experiment infrastructure): M = 16 controlled envs, K = 256
candidates, H = 4 steps (a 4,096-env planner sim, abs_pos, staged reward, no cameras).

  a  the fused call: mmx_mppi_plan with the library's noise
  b  the recipe it replaces, from entry points the parent commit has: restore(snap, src), torch sampling,
     rollout_actions with reward and done recorded, torch masking, softmax and the weighted mean (no host
     synchronisation either).  With --baseline-lib it runs on that library (e.g. the parent commit's build, the
     default library of a child process through MMX_LIB_PATH, as every figure under profiles/ was measured);
     without, on this one
  c  the rollout alone: rollout_actions, reward and done recorded, of the very candidates line a rolls out,
     from the same branched state (the branch is made before the timed call)

Every timed call does the same work: before it (untimed) the nominal plans are reset to the expert's action at
the snapshot, which also resets line a's call counter, so a and c step identical candidates and b candidates
of the same distribution (its own torch.randn).

A measurement is one line in one round: fresh sims (one planner sim alive at a time), the controlled env
advanced `ADVANCE` expert steps and snapshotted once, WARMUP untimed calls, then CALLS timed calls, each
between two events on the planner's stream and started on an idle device; the line's value in the round is
the median of its calls.  Five rounds, the lines one after another within a round, so drift hits all alike.
Reported: each line's median over the rounds and its spread (max - min), a - c (the planner's own share) and
the acceptance: median(a) <= median(b) + spread(b).  Exit status 1 when that does not hold.

  python tools/mppi_time.py [--baseline-lib PATH] [--out FILE]
"""
import argparse
import json
import os
import select
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from mujoco_manip_amd import _lib  # noqa: E402

M, K, H, A = 16, 256, 4, 4
N = M * K
ROUNDS, ADVANCE, WARMUP, CALLS = 5, 12, 3, 10
SIGMA, LOW, HIGH = (0.05, 0.05, 0.05, 0.6), (-0.5, 0.0, 0.24, 0.0), (0.5, 0.8, 0.60, 1.0)
TEMPERATURE, GAMMA, SEED = 0.01, 0.95, 42
CFG = dict(tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True, image_size=0, autoreset=False)


def controlled():
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(M, **CFG)
    env.reset(seed=[_lib.episode_seed(SEED, i) for i in range(M)])
    env.rollout_expert(ADVANCE)
    return env, env.snapshot(), env.expert_plan()


def timed_calls(f, between=None) -> float:
    """Median milliseconds of CALLS calls of f after WARMUP, each between two events, each from an idle device."""
    ms = []
    for k in range(WARMUP + CALLS):
        if between:
            between()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        if k >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def line_a():
    from mujoco_manip_amd.planner import MppiPlanner

    env, snap, a0 = controlled()
    p = MppiPlanner(env, K, H, SIGMA, temperature=TEMPERATURE, discount=GAMMA, seed=SEED, low=LOW, high=HIGH)
    ms = timed_calls(lambda: p.plan(snapshot=snap), between=lambda: p.reset(a0))
    p.close()
    env.close()
    return ms


def line_c():
    from mujoco_manip_amd.planner import MppiPlanner

    env, snap, a0 = controlled()
    p = MppiPlanner(env, K, H, SIGMA, temperature=TEMPERATURE, discount=GAMMA, seed=SEED, low=LOW, high=HIGH)
    p.reset(a0)
    p.plan(snapshot=snap)  # line a's candidates (call 0 after a reset), left in the planner's buffer
    sim, acts = p.sim_env.sim, p.buffers["actions"]
    src = (torch.arange(N, device=env.device, dtype=torch.int32) // K).contiguous()
    reward = torch.empty(H, N, device=env.device)
    done = torch.empty(H, N, 3, dtype=torch.int32, device=env.device)
    rec = _lib.MMXTrajectory()
    rec.reward, rec.done = reward.data_ptr(), done.data_ptr()
    ms = timed_calls(lambda: sim.rollout_actions(acts.data_ptr(), A, H, rec),
                     between=lambda: sim.restore(snap.data.data_ptr(), M, src.data_ptr()))
    p.close()
    env.close()
    return ms


class Recipe:
    """The planner sim, its record arrays and the torch side of line b."""

    def __init__(self):
        from mujoco_manip_amd.vec_env import PickPlaceVecEnv

        self.env, self.snap, a0 = controlled()
        dev = self.env.device
        self.sim_env = PickPlaceVecEnv(N, **CFG)
        self.sim_env.reset(seed=SEED)
        self.src = (torch.arange(N, device=dev, dtype=torch.int32) // K).contiguous()
        self.nominal0 = a0.clamp(torch.tensor(LOW, device=dev), torch.tensor(HIGH, device=dev)).expand(H, M, A).contiguous()
        self.nominal = self.nominal0
        self.sigma, self.low, self.high = (torch.tensor(v, device=dev) for v in (SIGMA, LOW, HIGH))
        self.reward = torch.empty(H, N, device=dev)
        self.done = torch.empty(H, N, 3, dtype=torch.int32, device=dev)
        self.rec = _lib.MMXTrajectory()
        self.rec.reward, self.rec.done = self.reward.data_ptr(), self.done.data_ptr()
        self.gamma = (GAMMA ** torch.arange(H, device=dev, dtype=torch.float32))[:, None]
        self.gen = torch.Generator(device=dev).manual_seed(SEED)

    def sample(self):
        eps = torch.randn(H, N, A, generator=self.gen, device=self.env.device)
        eps[:, ::K] = 0.0
        return torch.minimum(torch.maximum(self.nominal.repeat_interleave(K, dim=1) + self.sigma * eps, self.low), self.high)

    def restore(self):
        self.sim_env.sim.restore(self.snap.data.data_ptr(), M, self.src.data_ptr())

    def rollout(self):
        self.sim_env.sim.rollout_actions(self.actions.data_ptr(), A, H, self.rec)

    def reset(self):
        self.nominal = self.nominal0

    def step(self):
        self.restore()
        self.actions = self.sample()
        self.rollout()
        ended = (self.done[..., 0] | self.done[..., 1]) != 0
        alive = torch.ones_like(ended)
        alive[1:] = torch.cumsum(ended[:-1].int(), dim=0) == 0
        R = (self.gamma * self.reward * alive).sum(dim=0)
        w = torch.softmax(R.view(M, K) / TEMPERATURE, dim=1)
        new = torch.einsum("mk,tmka->tma", w, self.actions.view(H, M, K, A))
        self.nominal = torch.cat([new[1:], new[-1:]])
        return new[0]

    def close(self):
        self.sim_env.close()
        self.env.close()


def line_b():
    r = Recipe()
    ms = timed_calls(r.step, between=r.reset)
    r.close()
    return ms


def serve():
    """Line b on the library MMX_LIB_PATH names: one measurement per line read on stdin."""
    print("ready", flush=True)
    for _ in sys.stdin:
        print(json.dumps(line_b()), flush=True)


def reply(child, seconds=300.0) -> str:
    """The child's next line; a child that died or stays silent for `seconds` is an error, not a wait."""
    ready, _, _ = select.select([child.stdout], [], [], seconds)
    line = child.stdout.readline() if ready else ""
    if not line:
        status = child.poll()
        child.kill()
        raise RuntimeError("baseline child " + (f"exited with status {status}" if status is not None
                                                else f"gave no reply within {seconds:.0f} s"))
    return line.strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None, help="library of the baseline commit for line b")
    ap.add_argument("--out", default=None, help="file for the full result (the summary line is printed either way)")
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.serve:
        return serve()
    child = None
    if a.baseline_lib:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve"], stdin=subprocess.PIPE,
                                 stdout=subprocess.PIPE, text=True, env=dict(os.environ, MMX_LIB_PATH=os.path.abspath(a.baseline_lib)))
        assert reply(child) == "ready", "baseline child failed to start"
    ms = {"a": [], "b": [], "c": []}
    for _ in range(ROUNDS):
        ms["a"].append(line_a())
        if child:
            child.stdin.write("go\n")
            child.stdin.flush()
            ms["b"].append(float(json.loads(reply(child))))
        else:
            ms["b"].append(line_b())
        ms["c"].append(line_c())
    if child:
        child.stdin.close()
        child.wait(timeout=60)
    us = {ln: {"median": 1e3 * float(np.median(v)), "spread": 1e3 * (max(v) - min(v)), "rounds": [1e3 * x for x in v]}
          for ln, v in ms.items()}
    own = us["a"]["median"] - us["c"]["median"]
    res = {"shape": {"M": M, "K": K, "H": H, "A": A, "planner_envs": N}, "rounds": ROUNDS, "calls_per_round": CALLS,
           "warmup_calls": WARMUP, "unit": "microseconds per control step", "baseline_lib": a.baseline_lib, "lines": us,
           "planner_overhead_us": own, "planner_overhead_share_of_a": own / us["a"]["median"],
           "a_over_b": us["a"]["median"] / us["b"]["median"],
           "accepted": us["a"]["median"] <= us["b"]["median"] + us["b"]["spread"]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items() if k != "lines"}
                     | {"median_us": {ln: round(v["median"], 1) for ln, v in us.items()},
                        "spread_us": {ln: round(v["spread"], 1) for ln, v in us.items()}}))
    return 0 if res["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
