"""Random-shooting control of one env with a K-env planner sim: the worked example of INTEGRATION.md's
planner recipe (not a benchmark).

Every control step: snapshot the controlled env, start all K planner envs from that one record
(restore(snap, src=0)), roll K candidate action sequences out in one fused launch with only the reward
recorded, and apply the first action of the best one.  A candidate is a target near the end effector held
for the horizon with the gripper open or closed; the best candidate of the last step is kept among them.
Both sims share the configuration (the record carries state, not configuration) and run without
autoreset, so a candidate's return is the return the controlled env would collect.

  python tools/shooting_example.py [--candidates 256] [--horizon 4] [--steps 30] [--seed 0]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from mujoco_manip_amd import _lib  # noqa: E402
from mujoco_manip_amd.vec_env import PickPlaceVecEnv  # noqa: E402

LOW, HIGH = (-0.5, 0.0, 0.24), (0.5, 0.8, 0.60)  # abs_pos action box (gym_env.make_action_space)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=4)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--sigma", type=float, default=0.08, help="spread of the candidate targets around the end effector (m)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    K, H = a.candidates, a.horizon
    cfg = dict(tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True, image_size=0)
    env, planner = PickPlaceVecEnv(1, **cfg), PickPlaceVecEnv(K, **cfg)
    env.reset(seed=a.seed)
    planner.reset(seed=a.seed)
    gen = torch.Generator(device=env.device).manual_seed(a.seed)
    low, high = torch.tensor(LOW, device=env.device), torch.tensor(HIGH, device=env.device)
    best = None
    total, log = 0.0, []
    for t in range(a.steps):
        snap = env.snapshot()
        planner.restore(snap, src=0)  # one record to K envs: the branch
        ee = env.sim.view("kin", _lib.KIN_N)[0, :3]
        cand = torch.empty(K, 4, device=env.device)
        cand[:, :3] = torch.minimum(torch.maximum(ee + a.sigma * torch.randn(K, 3, generator=gen, device=env.device), low), high)
        cand[:, 3] = torch.randint(0, 2, (K,), generator=gen, device=env.device).float()
        if best is not None:
            cand[0] = best
        plans = cand.unsqueeze(0).expand(H, K, 4).contiguous()  # [H, K, 4]: the target held for the horizon
        returns = planner.rollout(plans, record=("reward",))["reward"].sum(dim=0)
        k = int(torch.argmax(returns).item())
        best = cand[k].clone()
        _, reward, terminated, truncated, info = env.step(best.unsqueeze(0))
        total += float(reward[0].item())
        log.append({"step": t, "reward": round(float(reward[0].item()), 4), "planned_return": round(float(returns[k].item()), 4),
                    "gripper": int(best[3].item())})
        if bool(terminated[0].item()) or bool(truncated[0].item()):
            break
    print(json.dumps({"task": env.tasks[0], "candidates": K, "horizon": H, "steps": len(log), "return": round(total, 4),
                      "success": bool(info["success"][0].item()), "last": log[-3:]}))
    env.close()
    planner.close()


if __name__ == "__main__":
    main()
