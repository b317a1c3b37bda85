"""What a closed-loop policy rollout costs (experiment infrastructure): C3's shape (4,096 envs, abs_pos, all tasks,
randomised, staged reward, no cameras), a tanh MLP 85 -> 256 -> 256 -> 4 behaviour-cloned from the on-device
expert as in tools/policy_example.py (1,024 envs x 300 expert steps, 300 Adam steps, seeded), deterministic.

  a  the loop it replaces: obs -> torch MLP -> clamp -> Sim.step, one launch per env step, no host wait.  With
     --baseline-lib it runs on that library (e.g. the parent commit's build, bound to the line's sims with lib=)
     in a child process, as every figure under profiles/ was measured; without, on this one
  b  rollout_policy with obs, reward and done recorded
  c  rollout(actions=...) replaying exactly the actions b recorded, with the same record

b and c follow identical trajectories (asserted on the final state), so b - c is the policy's own cost; a's
actions differ from b's in last bits, so its trajectory drifts from theirs: its spread over the rounds is reported.
The FSM-phase mix a policy induces sets the step cost, so a, b and c compare with each other only.

A measurement is one line in one round: a fresh env, the seeded reset, 120 * round env steps untimed under the
policy, an untimed window of each length, then a timed window of T = 20 and one of T = 100 env steps, each
between two events on the sim's stream, started on an idle device.  Five rounds, the lines one after another
within a round, so drift hits all alike; one sim alive at a time.  Reported: env steps/s per line and round,
b / a, (b - c) / b in time, b - c in microseconds per step of all envs, and the acceptance median(b) >=
median(a) - spread(a) (exit status 1 when it fails).

  python tools/policy_time.py [--baseline-lib PATH] [--envs 4096] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]
from mujoco_manip_amd.planner import action_box  # noqa: E402
from policy_example import SEED, cloned_policy, make_env  # noqa: E402

ROUNDS, ADVANCE, WARMUP, WINDOWS = 5, 120, (20, 100), (20, 100)
RECORD = ("obs", "reward", "done")


def timed(f) -> float:
    """Seconds of f on the current stream (the sim's), between two events, from an idle device."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


class TorchPolicy:
    """Line a's policy: the same weights through torch modules, with the device path's normalisation and clamp."""

    def __init__(self, arrays, device):
        t = {k: torch.as_tensor(v, device=device) for k, v in arrays.items()}
        self.W = [t[f"W{k}"] for k in range(3)]
        self.b = [t[f"b{k}"] for k in range(3)]
        self.shift, self.scale, self.low, self.high = t["shift"], t["scale"], t["low"], t["high"]

    @torch.no_grad()
    def __call__(self, obs):
        x = (obs - self.shift) * self.scale
        for k in range(2):
            x = torch.tanh(torch.addmm(self.b[k], x, self.W[k].t()))
        return torch.clamp(torch.addmm(self.b[2], x, self.W[2].t()), self.low, self.high)


def loop_steps(env, pol, T):
    for _ in range(T):
        a = pol(env._obs)
        env.sim.step(a.data_ptr(), 4)
        env._last_action = a  # alive until the next step is queued (same stream: ordered)


def run_round(line, r, n, arrays, replay=None, lib=None):
    """One measurement of `line` on the build `lib` of the library -> ({T: seconds}, digest of the final qpos, the
    recorded actions (line b))."""
    env = make_env(n, lib=lib)
    mlp = None
    if line == "a":
        pol = TorchPolicy(arrays, env.device)
        step = lambda T, acts: loop_steps(env, pol, T)  # noqa: E731
    else:
        from mujoco_manip_amd.policy import MlpPolicy

        mlp = MlpPolicy([(arrays[f"W{k}"], arrays[f"b{k}"]) for k in range(3)], obs_shift=arrays["shift"],
                        obs_scale=arrays["scale"], low=arrays["low"], high=arrays["high"]).bind(env)
        if line == "b":
            step = lambda T, acts: env.rollout_policy(mlp, T, record=RECORD)  # noqa: E731
        else:
            step = lambda T, acts: env.rollout(acts, record=RECORD)  # noqa: E731
    off = r * ADVANCE
    if off:  # the same states ahead of every line's windows (line a: its own loop, last bits apart)
        step(off, None) if line == "a" else env.rollout_policy(mlp, off, record=())
    secs, kept, out = {}, [], None
    for w, T in enumerate(WARMUP + WINDOWS):
        acts = replay[w] if line == "c" else None

        def window():
            nonlocal out
            out = step(T, acts)

        t = timed(window)
        if line == "b":
            kept.append(out["actions"])
        if w >= len(WARMUP):
            secs[T] = t
    env.synchronize()
    digest = hashlib.sha256(env.qpos.cpu().numpy().tobytes()).hexdigest()
    if mlp is not None:
        mlp.close()
    env.close()
    return secs, digest, kept


def serve(lib, arrays_file, n):
    """Line a on a library of another commit (_lib.load binds the calls it has; only create / reset / step /
    synchronize are used): serves round numbers on stdin with run_round's result."""
    arrays = dict(np.load(arrays_file))
    print("ready", flush=True)
    for req in sys.stdin:
        secs, digest, _ = run_round("a", int(req), n, arrays, lib=lib)
        print(json.dumps([secs, digest]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--baseline-lib", default=None, help="library of the baseline commit for line a")
    ap.add_argument("--out", default=None, help="file for the full result (the summary line is printed either way)")
    ap.add_argument("--serve", nargs=2, metavar=("LIB", "ARRAYS"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.serve:
        return serve(a.serve[0], a.serve[1], a.envs)
    n = a.envs
    net, shift, scale, loss = cloned_policy()
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    low, high = action_box("abs_pos")
    arrays = {"shift": shift, "scale": scale, "low": torch.tensor(low), "high": torch.tensor(high)}
    for k, m in enumerate(lin):
        arrays[f"W{k}"], arrays[f"b{k}"] = m.weight, m.bias
    arrays = {k: v.detach().cpu().numpy().astype(np.float32) for k, v in arrays.items()}
    del net, lin
    torch.cuda.empty_cache()

    child = None
    if a.baseline_lib:
        fd, arrays_file = tempfile.mkstemp(suffix=".npz")
        os.close(fd)
        np.savez(arrays_file, **arrays)
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--envs", str(n), "--serve",
                                  os.path.abspath(a.baseline_lib), arrays_file], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                 text=True)
        assert child.stdout.readline().strip() == "ready", "baseline child failed to start"
        os.unlink(arrays_file)
    lines = ["a", "b", "c"]
    secs_all = {ln: {T: [] for T in WINDOWS} for ln in lines}
    for r in range(ROUNDS):
        final, replay = {}, None
        for ln in lines:
            if ln == "a" and child:
                child.stdin.write(f"{r}\n")
                child.stdin.flush()
                secs, final[ln] = json.loads(child.stdout.readline())
                secs = {int(T): t for T, t in secs.items()}
            else:
                secs, final[ln], kept = run_round(ln, r, n, arrays, replay)
                replay = kept if ln == "b" else replay
            for T in WINDOWS:
                secs_all[ln][T].append(secs[T])
        assert final["b"] == final["c"], f"the replay ended in another state than the policy rollout: {final}"
    if child:
        child.stdin.close()
        child.wait(timeout=60)

    res = {"envs": n, "rounds": ROUNDS, "advance_steps_per_round": ADVANCE, "warmup_windows": list(WARMUP),
           "windows": list(WINDOWS), "unit": "env steps/s", "baseline_lib": a.baseline_lib, "record": list(RECORD),
           "policy": {"layers": [85, 256, 256, 4], "activation": "tanh", "deterministic": True,
                      "weights": "behaviour-cloned from the expert (tools/policy_example.cloned_policy, seed %d)" % SEED,
                      "fit_last_loss": loss},
           "lines": {}, "ratios": {}, "acceptance": {}}
    ok = True
    for T in WINDOWS:
        rate = {ln: [n * T / s for s in secs_all[ln][T]] for ln in lines}
        for ln in lines:
            v = rate[ln]
            res["lines"].setdefault(ln, {})[f"T{T}"] = {"min": min(v), "median": float(np.median(v)), "max": max(v), "rounds": v}
        b_a = [b / x for b, x in zip(rate["b"], rate["a"])]
        share = [(sb - sc) / sb for sb, sc in zip(secs_all["b"][T], secs_all["c"][T])]
        us = [(sb - sc) / T * 1e6 for sb, sc in zip(secs_all["b"][T], secs_all["c"][T])]
        res["ratios"][f"T{T}"] = {"policy_us_per_step_of_all_envs": {"min": min(us), "median": float(np.median(us)), "max": max(us),
                                                                     "rounds": us},
                                  "b_over_a": {"min": min(b_a), "median": float(np.median(b_a)), "max": max(b_a), "rounds": b_a},
                                  "policy_share_of_b": {"min": min(share), "median": float(np.median(share)), "max": max(share),
                                                        "rounds": share}}
        spread_a = max(rate["a"]) - min(rate["a"])
        holds = float(np.median(rate["b"])) >= float(np.median(rate["a"])) - spread_a
        res["acceptance"][f"T{T}"] = {"median_b": float(np.median(rate["b"])), "median_a": float(np.median(rate["a"])),
                                     "spread_a": spread_a, "holds": bool(holds)}
        ok = ok and holds
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"median": {ln: {k: round(v["median"]) for k, v in d.items()} for ln, d in res["lines"].items()},
                      "ratios": {T: {k: [round(v[m], 4) for m in ("min", "median", "max")] for k, v in d.items()}
                                 for T, d in res["ratios"].items()},
                      "acceptance": {T: d["holds"] for T, d in res["acceptance"].items()}}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
