"""What the expert's shadow costs a closed-loop policy rollout (experiment infrastructure): C3's shape (4,096 envs,
abs_pos, all tasks, randomised, staged reward, no cameras), the tanh MLP 85 -> 256 -> 256 -> 4 behaviour-cloned from
the on-device expert of tools/policy_example.py, deterministic.

  p  rollout_policy with obs, reward and done recorded (mmx_rollout_policy)
  d  rollout_dagger with beta = 0 and no takeover, the same record plus obs_in, expert_action and gate
     (mmx_rollout_dagger): the learner acts at every step, so d follows p's trajectory exactly (asserted on the
     final state) and d - p is what lane 0's expert plan, Philox block and extra record rows cost

The two lines differ in one more thing than the kernel: the FSM state moves under d (the expert plans) and stays idle
under p, and the step launches' dispatch order sorts by it.  A mixture (beta > 0) follows other trajectories, whose
FSM-phase mix sets the step cost, so it compares with nothing here and is not timed.

A measurement is one line in one round: a fresh env, the seeded reset, 120 * round env steps untimed under the line's
own call, one untimed window, then WINDOWS timed windows of T = 64 env steps, each between two events on the sim's
stream, started on an idle device.  Five rounds; in a round every line is measured twice, in the order p d d p, so
drift hits both alike; one sim alive at a time.  The states a window starts from are the same for both lines and for
both repeats (same seeds, same actions), and they set the window's cost: windows differ from each other by far more
than the lines do, so everything is compared per (round, window).  Reported: seconds per window per line, round and
repeat; each line's run-to-run spread, |repeat 1 - repeat 0| / their mean per (round, window); and the paired
difference (d - p) / p of the repeats' means per (round, window), beside that spread.

  python tools/dagger_time.py [--envs 4096] [--steps 64] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]
from mujoco_manip_amd.planner import action_box  # noqa: E402
from policy_example import SEED, cloned_policy, make_env  # noqa: E402
from policy_time import timed  # noqa: E402

ROUNDS, ADVANCE, WINDOWS = 5, 120, 3
RECORD = ("obs", "reward", "done")
DAGGER_RECORD = RECORD + ("obs_in", "expert_action", "gate")


def run_round(line, r, n, T, net, shift, scale):
    """One measurement of `line` -> (seconds of each timed window, digest of the final qpos)."""
    from mujoco_manip_amd.policy import MlpPolicy

    low, high = action_box("abs_pos")
    env = make_env(n)
    mlp = MlpPolicy.from_torch(net, obs_shift=shift, obs_scale=scale, low=low, high=high).bind(env)
    if line == "p":
        step = lambda k, record: env.rollout_policy(mlp, k, record=record)  # noqa: E731
        record = RECORD
    else:
        step = lambda k, record: env.rollout_dagger(mlp, k, beta=0.0, takeover_dist=0.0, record=record)  # noqa: E731
        record = DAGGER_RECORD
    if r:
        step(r * ADVANCE, ())
    step(T, record)  # warm-up: the window's shape
    secs = [timed(lambda: step(T, record)) for _ in range(WINDOWS)]
    env.synchronize()
    digest = hashlib.sha256(env.qpos.cpu().numpy().tobytes()).hexdigest()
    mlp.close()
    env.close()
    return secs, digest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default=None, help="file for the full result (the summary line is printed either way)")
    a = ap.parse_args()
    n, T = a.envs, a.steps
    net, shift, scale, loss = cloned_policy()
    secs = {"p": [], "d": []}  # [round][repeat][window]
    for r in range(ROUNDS):
        final, got = [], {"p": [], "d": []}
        for ln in ("p", "d", "d", "p"):
            s, digest = run_round(ln, r, n, T, net, shift, scale)
            got[ln].append(s)
            final.append(digest)
        assert len(set(final)) == 1, f"rollout_dagger(beta=0) ended in another state than rollout_policy: {final}"
        for ln in got:
            secs[ln].append(got[ln])
    t = {ln: np.array(v) for ln, v in secs.items()}  # [ROUNDS, 2, WINDOWS]

    def summary(x):
        return {"min": float(x.min()), "median": float(np.median(x)), "max": float(x.max())}

    res = {"envs": n, "steps_per_window": T, "rounds": ROUNDS, "repeats_per_round": 2, "windows_per_round": WINDOWS,
           "advance_steps_per_round": ADVANCE, "unit": "seconds per window", "record": {"p": list(RECORD), "d": list(DAGGER_RECORD)},
           "policy": {"layers": [85, 256, 256, 4], "activation": "tanh", "deterministic": True,
                      "weights": "behaviour-cloned from the expert (tools/policy_example.cloned_policy, seed %d)" % SEED,
                      "fit_last_loss": loss},
           "lines": {}}
    for ln, x in t.items():
        spread = np.abs(x[:, 1] - x[:, 0]) / x.mean(axis=1)
        res["lines"][ln] = {"seconds": summary(x), "env_steps_per_s_at_median": n * T / float(np.median(x)),
                            "run_to_run_spread_relative": summary(spread), "rounds": x.tolist()}
    paired = (t["d"].mean(axis=1) - t["p"].mean(axis=1)) / t["p"].mean(axis=1)
    worst_spread = max(res["lines"][ln]["run_to_run_spread_relative"]["max"] for ln in t)
    res["d_minus_p_relative"] = dict(summary(paired), per_round_and_window=paired.tolist(), largest_run_to_run_spread=worst_spread,
                                     inside_spread=bool(np.abs(paired).max() <= worst_spread))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"median_s": {ln: round(d["seconds"]["median"], 6) for ln, d in res["lines"].items()},
                      "run_to_run_spread_relative": {ln: {k: round(v, 5) for k, v in d["run_to_run_spread_relative"].items()}
                                                     for ln, d in res["lines"].items()},
                      "d_minus_p_relative": {k: (round(v, 5) if isinstance(v, float) else v) for k, v in res["d_minus_p_relative"].items()
                                             if k != "per_round_and_window"}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
