"""What a policy-gradient fit costs on the device against the MSE fit it shares its step with and against the torch
loop it replaces (experiment infrastructure; no gate).  tools/fit_time.py's shape and protocol: the tanh MLP
85 -> 256 -> 256 -> 4, batch 8192, 300 Adam steps on 300 k samples (seeded random observations, mean_old from a
perturbed copy of the net, normal noise and advantages: the cost does not depend on the data).

  a  policy.fit_pg(x, mean_old, noise, adv, 300): mmx_policy_fit_pg, four launches per step, weights updated in place
  b  policy.fit(x, y, 300): mmx_policy_fit, three launches per step: the yardstick for what the objective costs over
     the shared gradient GEMM and update
  c  the torch loop: autograd of the same surrogate on minibatches drawn with torch.randint, torch.optim.Adam, then
     policy.load(net) (the upload a round of training pays for new weights on the device)

A measurement is one line: an untimed warm-up call of the same shape, then the timed call between two events on the
sim's stream from an idle device.  Five rounds, each in the order a b c c b a, so drift hits all alike.  Reported:
seconds per line, round and repeat, each line's run-to-run spread |repeat 1 - repeat 0| / mean, and a / b and a / c of
the medians.

  python tools/pg_time.py [--pairs 300000] [--batch 8192] [--steps 300] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]
from policy_example import make_env  # noqa: E402
from policy_time import timed  # noqa: E402

ROUNDS = 5
CLIP = 0.2


def torch_pg(net, xn, mean_old, noise, adv, std, steps, batch, lr=3e-4):
    """The loop fit_pg replaces: the clipped surrogate of the pre-clamp sample's density ratio, Adam."""
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    n = xn.shape[0]
    last = None
    for _ in range(steps):
        idx = torch.randint(0, n, (batch,), device=xn.device)
        z = noise[idx]
        zn = (mean_old[idx] + std * z - net(xn[idx])) / std
        r = torch.exp(0.5 * (z * z - zn * zn).sum(1))
        A = adv[idx]
        loss = -torch.minimum(r * A, torch.clamp(r, 1 - CLIP, 1 + CLIP) * A).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        last = loss
    return float(last.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=300_000)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", default=None, help="file for the full result (the summary line is printed either way)")
    a = ap.parse_args()
    from mujoco_manip_amd.policy import MlpPolicy

    if not torch.cuda.is_available():
        raise SystemExit("pg_time.py measures on the GPU: none found")
    nn = torch.nn
    env = make_env(16)
    torch.manual_seed(0)
    x = torch.randn(a.pairs, 85, device=env.device)
    shift, scale = x.mean(0), 1.0 / x.std(0)
    log_std = torch.full((4,), -0.5)
    std = log_std.exp().to(env.device)

    def fresh_net():
        torch.manual_seed(1)
        return nn.Sequential(nn.Linear(85, 256), nn.Tanh(), nn.Linear(256, 256), nn.Tanh(), nn.Linear(256, 4)).to(env.device)

    with torch.no_grad():
        old = fresh_net()
        for q in old.parameters():
            q.add_(0.02 * torch.randn_like(q))
        xn = ((x - shift) * scale).contiguous()
        mean_old = old(xn).contiguous()
        y = mean_old.clone()
    noise = torch.randn(a.pairs, 4, device=env.device)
    adv = torch.randn(a.pairs, device=env.device)

    def bound():
        return MlpPolicy.from_torch(fresh_net(), obs_shift=shift, obs_scale=scale, log_std=log_std).bind(env)

    def line_a():
        policy = bound()
        policy.fit_pg(x, mean_old, noise, adv, a.steps, clip=CLIP, batch=a.batch)  # warm-up: the workspace is allocated here
        out = []
        secs = timed(lambda: out.append(policy.fit_pg(x, mean_old, noise, adv, a.steps, clip=CLIP, batch=a.batch, reset_optimizer=True)))
        last = float(out[0][-1, 0])
        policy.close()
        return secs, last

    def line_b():
        policy = bound()
        policy.fit(x, y, a.steps, batch=a.batch)
        out = []
        secs = timed(lambda: out.append(policy.fit(x, y, a.steps, batch=a.batch, reset_optimizer=True)))
        last = float(out[0][-1])
        policy.close()
        return secs, last

    def line_c():
        policy = bound()

        def once(net):
            last = torch_pg(net, xn, mean_old, noise, adv, std, a.steps, a.batch)
            policy.load(net)
            env.synchronize()
            return last

        once(fresh_net())  # warm-up
        net, out = fresh_net(), []
        secs = timed(lambda: out.append(once(net)))
        policy.close()
        return secs, out[0]

    lines = {"a": line_a, "b": line_b, "c": line_c}
    secs, lasts = {ln: [] for ln in lines}, {ln: [] for ln in lines}
    for _ in range(ROUNDS):
        got = {ln: [] for ln in lines}
        for ln in ("a", "b", "c", "c", "b", "a"):
            s, last = lines[ln]()
            got[ln].append(s)
            lasts[ln].append(last)
        for ln in got:
            secs[ln].append(got[ln])
    env.close()
    t = {ln: np.array(v) for ln, v in secs.items()}  # [ROUNDS, 2]
    res = {"pairs": a.pairs, "batch": a.batch, "adam_steps": a.steps, "layers": [85, 256, 256, 4], "activation": "tanh", "rounds": ROUNDS,
           "repeats_per_round": 2, "unit": "seconds per fit", "what": {"a": "fit_pg", "b": "fit (MSE)", "c": "torch autograd + Adam + load"},
           "lines": {}}
    for ln, v in t.items():
        spread = np.abs(v[:, 1] - v[:, 0]) / v.mean(axis=1)
        res["lines"][ln] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
                            "seconds_per_adam_step_at_median": float(np.median(v)) / a.steps,
                            "run_to_run_spread_relative_max": float(spread.max()), "rounds": v.tolist(), "last": lasts[ln]}
    med = {ln: res["lines"][ln]["median"] for ln in lines}
    res["fit_pg_over_fit_at_medians"] = med["a"] / med["b"]
    res["fit_pg_over_torch_at_medians"] = med["a"] / med["c"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"median_s": {ln: round(d["median"], 5) for ln, d in res["lines"].items()},
                      "spread_max": {ln: round(d["run_to_run_spread_relative_max"], 4) for ln, d in res["lines"].items()},
                      "fit_pg_over_fit": round(res["fit_pg_over_fit_at_medians"], 3),
                      "fit_pg_over_torch": round(res["fit_pg_over_torch_at_medians"], 3)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
