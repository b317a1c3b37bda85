"""Generates tests/golden/render_states.npz: the states the flat camera images are pinned on per pixel
(tests/test_render_flat_pixels.py).

Run on the CPU, from the repository root (the fp64 oracle only; no GPU, nothing of the reference):

    python tests/golden/make_render_states.py

Two fp64 oracle expert episodes from the keyframe, stepped as the environment steps them (fsm_plan(16),
fsm_actuate, 16 x mj_step per env step), one task each so that two cube colours and two bins take part:
red cube -> red bin and blue cube -> green bin.  Of each FSM phase asked for, the state in the middle of
the phase's env steps.  The file holds `qpos` [n, 30] float32 (what the tests hand to set_state and to the
oracle alike), `labels` [n] and `phase` [n] (the FSM state at the snapshot, -1 for the two keyframes).

  keyframe          the model's keyframe
  keyframe_turned   the keyframe with joint 0 at -1.5708: the arm turned away, nothing occluded
  pre_grasp         red -> red, moving above the cube
  close_gripper     red -> red, the fingers closing on the cube
  held              blue -> green, move-to-bin with the cube held: the wrist camera sees its faces close up
  lower_to_bin      blue -> green, the held cube going down into the bin
  retreat           red -> red, the cube lying in the bin, the arm on its way back
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "oracle"))

S_PRE_GRASP, S_CLOSE_GRIPPER, S_MOVE_TO_BIN, S_LOWER_TO_BIN, S_RETREAT, S_DONE = 1, 3, 5, 7, 9, 10  # oracle/or_task.c
RED, GREEN, BLUE = 0, 1, 2


def episode(task):
    """[(FSM state, qpos)] after every env step of one expert episode of `task` from the keyframe."""
    import oracle_py as O

    e = O.OracleEnv()
    e.reset_keyframe()
    e.fsm_init([task])
    out = []
    for _ in range(2000):
        e.fsm_plan(16)
        e.fsm_actuate()
        for _ in range(16):
            e.mj_step()
        st = e.fsm_get()["state"]
        if st == S_DONE:
            break
        out.append((st, e.get_state()[0].copy()))
    return out


def middle_of(ep, phase):
    idx = [i for i, (st, _) in enumerate(ep) if st == phase]
    assert idx, f"the episode never reaches FSM state {phase}"
    return ep[idx[len(idx) // 2]][1]


def main():
    key = np.array(json.load(open(os.path.join(REPO, "mujoco_manip_amd", "model", "panda_pickplace.json")))["key_qpos"], float)
    turned = key.copy()
    turned[0] = -1.5708
    a, b = episode((RED, RED)), episode((BLUE, GREEN))
    states = [("keyframe", -1, key), ("keyframe_turned", -1, turned),
              ("pre_grasp", S_PRE_GRASP, middle_of(a, S_PRE_GRASP)),
              ("close_gripper", S_CLOSE_GRIPPER, middle_of(a, S_CLOSE_GRIPPER)),
              ("held", S_MOVE_TO_BIN, middle_of(b, S_MOVE_TO_BIN)),
              ("lower_to_bin", S_LOWER_TO_BIN, middle_of(b, S_LOWER_TO_BIN)),
              ("retreat", S_RETREAT, middle_of(a, S_RETREAT))]
    for name, ph, q in states:
        print(f"{name:16s} phase {ph:2d} arm {np.round(q[:7], 3).tolist()} cubes z {np.round(q[[11, 18, 25]], 3).tolist()}")
    np.savez_compressed(os.path.join(HERE, "render_states.npz"), qpos=np.stack([q for _, _, q in states]).astype(np.float32),
                        labels=np.array([n for n, _, _ in states]), phase=np.array([p for _, p, _ in states], np.int32))


if __name__ == "__main__":
    main()
