"""What a fit of the MLP policy costs on the device against the torch loop it replaces (experiment infrastructure; no
gate).  The DAgger example's shape: the tanh MLP 85 -> 256 -> 256 -> 4, batch 8192, 300 Adam steps on 300 k pairs
(seeded random observations, targets from a random teacher: the cost does not depend on the data).

  a  policy.fit(x, y, 300): mmx_policy_fit, three launches per step, the weights updated in place
  b  tools/dagger_example.train(net, (x - shift) * scale, y, 300) + MlpPolicy.from_torch(net).bind(env) + close: what a
     round of the example pays for new weights on the device (the normalisation of x included, as the example does it)

A measurement is one line: an untimed warm-up call of the same shape, then the timed call between two events on the
sim's stream from an idle device (b's host work, the re-creation included, lies between the events; its end is the
upload's own synchronisation).  Five rounds, each in the order a b b a, so drift hits both alike.  Reported: seconds
per line, round and repeat, each line's run-to-run spread |repeat 1 - repeat 0| / mean, and a / b of the medians.

  python tools/fit_time.py [--pairs 300000] [--batch 8192] [--steps 300] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]
from dagger_example import train  # noqa: E402
from policy_example import make_env  # noqa: E402
from policy_time import timed  # noqa: E402

ROUNDS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=300_000)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", default=None, help="file for the full result (the summary line is printed either way)")
    a = ap.parse_args()
    from mujoco_manip_amd.policy import MlpPolicy

    if not torch.cuda.is_available():
        raise SystemExit("fit_time.py measures on the GPU: none found")
    nn = torch.nn
    env = make_env(16)
    torch.manual_seed(0)
    x = torch.randn(a.pairs, 85, device=env.device)
    shift, scale = x.mean(0), 1.0 / x.std(0)
    teacher = nn.Sequential(nn.Linear(85, 64), nn.Tanh(), nn.Linear(64, 4)).to(env.device)
    with torch.no_grad():
        y = teacher(x).contiguous()

    def fresh_net():
        torch.manual_seed(1)
        return nn.Sequential(nn.Linear(85, 256), nn.Tanh(), nn.Linear(256, 256), nn.Tanh(), nn.Linear(256, 4)).to(env.device)

    def line_a():
        policy = MlpPolicy.from_torch(fresh_net(), obs_shift=shift, obs_scale=scale).bind(env)
        policy.fit(x, y, a.steps, batch=a.batch)  # warm-up: the workspace is allocated here
        loss = []
        secs = timed(lambda: loss.append(policy.fit(x, y, a.steps, batch=a.batch, reset_optimizer=True)))
        last = float(loss[0][-1])
        policy.close()
        return secs, last

    def line_b():
        def once(net):
            last = train(net, (x - shift) * scale, y, a.steps, batch=a.batch)
            policy = MlpPolicy.from_torch(net, obs_shift=shift, obs_scale=scale).bind(env)
            env.synchronize()
            policy.close()
            return last

        once(fresh_net())  # warm-up
        net, loss = fresh_net(), []
        secs = timed(lambda: loss.append(once(net)))
        return secs, loss[0]

    secs, losses = {"a": [], "b": []}, {"a": [], "b": []}
    for _ in range(ROUNDS):
        got = {"a": [], "b": []}
        for ln in ("a", "b", "b", "a"):
            s, last = (line_a if ln == "a" else line_b)()
            got[ln].append(s)
            losses[ln].append(last)
        for ln in got:
            secs[ln].append(got[ln])
    env.close()
    t = {ln: np.array(v) for ln, v in secs.items()}  # [ROUNDS, 2]
    res = {"pairs": a.pairs, "batch": a.batch, "adam_steps": a.steps, "layers": [85, 256, 256, 4], "activation": "tanh", "rounds": ROUNDS,
           "repeats_per_round": 2, "unit": "seconds per fit", "lines": {}}
    for ln, v in t.items():
        spread = np.abs(v[:, 1] - v[:, 0]) / v.mean(axis=1)
        res["lines"][ln] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
                            "seconds_per_adam_step_at_median": float(np.median(v)) / a.steps,
                            "run_to_run_spread_relative_max": float(spread.max()), "rounds": v.tolist(), "last_loss": losses[ln]}
    res["a_over_b_at_medians"] = res["lines"]["a"]["median"] / res["lines"]["b"]["median"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"median_s": {ln: round(d["median"], 5) for ln, d in res["lines"].items()},
                      "spread_max": {ln: round(d["run_to_run_spread_relative_max"], 4) for ln, d in res["lines"].items()},
                      "a_over_b": round(res["a_over_b_at_medians"], 3)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
