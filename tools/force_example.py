"""Contact forces through an expert episode: after every env step the grip force of both fingers (`touch`) and
the net contact wrench on the cube being carried, from PickPlaceVecEnv.contact_forces() (mmx_contact_forces: the
forward solve and mj_contactForce of the current state, as a pass of its own).  What a loop of
mujoco.mj_contactForce(model, data, i, out) over data.contact gives after env.step() in the reference.

  python tools/force_example.py [--steps 90] [--task obj_red bin_red]
  python tools/force_example.py --time 4096     the pass beside one env step on the C3 shape (event-timed)
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from mujoco_manip_amd import _lib  # noqa: E402
from mujoco_manip_amd.constants import OBJECTS  # noqa: E402
from mujoco_manip_amd.vec_env import PickPlaceVecEnv  # noqa: E402

FSM = ("idle", "pre_grasp", "grasp", "close_gripper", "lift", "move_to_bin", "settle_at_bin", "lower_to_bin", "release",
       "retreat", "done")


def episode(steps, task):
    env = PickPlaceVecEnv(1, task=tuple(task), action_mode="abs_pos", reward_type="staged", image_size=0)
    env.reset(seed=0)
    body = _lib.FORCE_BODIES.index(16 + OBJECTS.index(task[0]))
    print(f"{'step':>4} {'phase':<13} {'ncon':>4} {'touch L':>9} {'touch R':>9}   force on {task[0]} (N)          torque (N m)")
    for k in range(steps):
        env.step(env.expert_plan())
        f = env.contact_forces()
        st = int(env.fsm_state[0].item())
        w = f["body_wrench"][0, body].tolist()
        t = f["touch"][0].tolist()
        print(f"{k:4d} {FSM[min(st, 10)]:<13} {int(f['solve'][0, 0].item()):4d} {t[0]:9.4f} {t[1]:9.4f}   "
              f"{w[0]:8.4f} {w[1]:8.4f} {w[2]:8.4f}   {w[3]:9.6f} {w[4]:9.6f} {w[5]:9.6f}")
        if st == 10:
            break
    env.close()


def timed(env, f, reps):
    """Milliseconds per call of `reps` back-to-back calls between two events on the sim's stream."""
    f()
    env.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def timing(n):
    env = PickPlaceVecEnv(n, tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True,
                          autoreset=True, image_size=0)
    env.reset(seed=[_lib.episode_seed(42, i) for i in range(n)])
    env.rollout_expert(40)  # the envs spread over the approach and grasp phases
    action = env.expert_plan(16)
    snap = env.snapshot()
    for r in range(5):
        env.restore(snap)
        force = timed(env, env.sim.contact_forces, 20)
        step = timed(env, lambda: env.sim.step(action.data_ptr(), 4), 10)
        print(f"round {r}: contact_forces {force:.4f} ms, env step {step:.4f} ms, ratio 1 / {step / force:.1f}  (N = {n})")
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=90)
    ap.add_argument("--task", nargs=2, default=["obj_red", "bin_red"])
    ap.add_argument("--time", type=int, default=0, metavar="N")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("force_example.py needs the MI355X")
    timing(a.time) if a.time else episode(a.steps, a.task)


if __name__ == "__main__":
    main()
