"""MPPI control of M envs with one planner sim of M x K envs: the worked example of INTEGRATION.md's planner
section on the device-side call (not a benchmark).

Every control step is one library call (MppiPlanner.plan -> mmx_mppi_plan): sample K candidate action
sequences around each env's nominal plan, start each candidate's planner env from its env's snapshot record,
roll all of them out for H steps in fused launches, weight them by their returns and shift the plans.  The
loop never reads a value back: rewards and the done flags are accumulated on the device and copied once at
the end.  A candidate stops collecting reward when its episode ends, and an env whose episode has ended keeps
its last action's plan but no longer counts.

  python tools/mppi_example.py [--envs 4] [--candidates 256] [--horizon 4] [--steps 30] [--seed 0]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from mujoco_manip_amd.planner import MppiPlanner  # noqa: E402
from mujoco_manip_amd.vec_env import PickPlaceVecEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--candidates", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=4)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--sigma", type=float, default=0.05, help="spread of the candidate targets around the nominal (m)")
    ap.add_argument("--temperature", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    env = PickPlaceVecEnv(a.envs, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          image_size=0)
    env.reset(seed=a.seed)
    planner = MppiPlanner(env, a.candidates, a.horizon, (a.sigma, a.sigma, a.sigma, 0.6), temperature=a.temperature,
                          noise_beta=0.5, seed=a.seed)
    # the first nominal plan: hold the end effector where it is, gripper open
    start = torch.cat([env.sim.view("kin", 63)[:, :3], torch.ones(a.envs, 1, device=env.device)], dim=1)
    planner.reset(start)
    total = torch.zeros(a.envs, device=env.device)
    alive = torch.ones(a.envs, dtype=torch.bool, device=env.device)
    success = torch.zeros(a.envs, dtype=torch.bool, device=env.device)
    planned = torch.zeros(a.envs, device=env.device)
    for _ in range(a.steps):
        action = planner.plan()
        planned = planner.buffers["returns"].view(a.envs, a.candidates).amax(dim=1)
        _, reward, terminated, truncated, info = env.step(action)
        total += reward * alive
        success |= info["success"] & alive
        alive &= ~(terminated | truncated)
    torch.cuda.synchronize()  # the only wait: everything above was queued
    print(json.dumps({"tasks": env.tasks, "candidates": a.candidates, "horizon": a.horizon, "steps": a.steps,
                      "returns": [round(v, 4) for v in total.tolist()], "success": success.tolist(),
                      "last_planned_return": [round(v, 4) for v in planned.tolist()]}))
    planner.close()
    env.close()


if __name__ == "__main__":
    main()
