"""DAgger on the device (an example, not a benchmark and not a criterion: nobody had measured what success rates
the rounds reach; CHANGELOG.md holds the table of one run).

  1. expert rollouts: (observation, action) pairs of the on-device FSM expert (tools/policy_example.expert_pairs);
  2. behaviour cloning: a small tanh torch.nn.Sequential fitted to them (the observation standardised per entry, the
     normalisation fixed from here on);
  3. k rounds of MlpPolicy.from_torch(net) -> env.rollout_dagger(policy, steps, beta = beta0 * decay^round): the
     learner, or per step and env with probability beta the expert, drives the envs; the expert labels every visited
     state inside the launch -> DaggerBuffer.add -> the same net trained further on the aggregate (the expert's own
     pairs included);
  4. before the first round and after every round, the learner alone (rollout_policy on a fresh, identically seeded
     env): episodes ended, ended in success and ended with the cube in its bin, from the sticky `episodes` /
     `successes` / `placed` counters of episode_i, printed as a table beside the expert's own line.  Without the
     expert's FSM an episode ends on termination or at the time limit alone (500 steps), so the learner runs past it.

--fit torch (the default: the table stays comparable with CHANGELOG.md's) trains the net with torch.optim.Adam and
makes a new device policy of it every round; --fit device keeps ONE bound MlpPolicy through all rounds and
policy.fit(x, y, ...) (mmx_policy_fit: minibatch Adam steps in HIP, in place in the policy's device weights) replaces
train() and the re-creation: the loop then needs torch for its tensors only.

  python tools/dagger_example.py [--envs 1024] [--steps 300] [--rounds 4] [--beta0 0.5] [--decay 0.5]
                                 [--fit-steps 300] [--eval-steps 510] [--fit torch|device]
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]
from mujoco_manip_amd import _lib  # noqa: E402
from policy_example import SEED, expert_pairs, make_env  # noqa: E402

OK, PLACED, EPISODES = _lib.EPI["successes"], _lib.EPI["placed"], _lib.EPI["episodes"]


def train(net, x, y, steps, batch=8192, lr=1e-3, seed=0):
    """`steps` Adam steps of mean-squared error on (x, y), continuing `net`; returns the last loss."""
    gen = torch.Generator(device=x.device).manual_seed(seed)
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    loss = torch.zeros(())
    for _ in range(steps):
        idx = torch.randint(0, x.shape[0], (min(batch, x.shape[0]),), device=x.device, generator=gen)
        loss = ((net(x[idx]) - y[idx]) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    return float(loss.item())


def counters(env, base=(0, 0, 0)):
    """(successes, placed, episodes ended) since `base`."""
    env.synchronize()
    return tuple(int(env._epi[:, k].sum()) - b for k, b in zip((OK, PLACED, EPISODES), base))


def learner_alone(policy, n, steps, seed):
    """(successes, placed, episodes ended) of `steps` env steps of the learner (an unbound MlpPolicy) alone on a
    fresh env."""
    env = make_env(n, seed)
    base = counters(env)
    policy.bind(env)
    env.rollout_policy(policy, steps, record=())
    out = counters(env, base)
    policy.close()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--beta0", type=float, default=0.5)
    ap.add_argument("--decay", type=float, default=0.5)
    ap.add_argument("--fit-steps", type=int, default=300)
    ap.add_argument("--eval-steps", type=int, default=510)
    ap.add_argument("--fit", choices=("torch", "device"), default="torch")
    a = ap.parse_args()
    from mujoco_manip_amd.dagger import DaggerBuffer
    from mujoco_manip_amd.policy import MlpPolicy

    nn = torch.nn
    torch.manual_seed(0)
    env = make_env(a.envs)
    base = counters(env)
    obs_e, act_e = expert_pairs(env, a.steps)
    expert = counters(env, base)
    env.close()
    shift, sd = obs_e.mean(0), obs_e.std(0)
    scale = torch.where(sd > 1e-6, 1.0 / sd.clamp_min(1e-6), torch.zeros_like(sd))
    net = nn.Sequential(nn.Linear(_lib.NOBS, 256), nn.Tanh(), nn.Linear(256, 256), nn.Tanh(), nn.Linear(256, 4)).to(obs_e.device)
    device_fit = a.fit == "device"
    env = make_env(a.envs)  # the DAgger env runs on through the rounds: the learner's own state distribution
    # --fit device: the one policy object of the whole run, fitted in place
    policy = MlpPolicy.from_torch(net, obs_shift=shift, obs_scale=scale).bind(env) if device_fit else None

    def fit(x, y, seed):
        if device_fit:
            return float(policy.fit(x.contiguous(), y.contiguous(), a.fit_steps, seed=seed)[-1])
        return train(net, (x - shift) * scale, y, a.fit_steps, seed=seed)

    def learner():
        if device_fit:
            return MlpPolicy(policy.weights(), activation="tanh", obs_shift=shift, obs_scale=scale)
        return MlpPolicy.from_torch(net, obs_shift=shift, obs_scale=scale)

    loss = fit(obs_e, act_e, 0)
    rows = [("BC", "-", obs_e.shape[0], loss, "-", *learner_alone(learner(), a.envs, a.eval_steps, SEED + 1))]
    buf = DaggerBuffer()
    for k in range(a.rounds):
        beta = a.beta0 * a.decay ** k
        if not device_fit:
            policy = MlpPolicy.from_torch(net, obs_shift=shift, obs_scale=scale).bind(env)
        rec = env.rollout_dagger(policy, a.steps, beta=beta, call=k)
        env.synchronize()
        if not device_fit:
            policy.close()
        buf.add(rec)
        obs_d, act_d = buf.tensors()
        x, y = torch.cat([obs_e, obs_d]), torch.cat([act_e, act_d])
        loss = fit(x, y, k + 1)
        share = float((rec["gate"] != 0).float().mean())
        rows.append((f"round {k + 1}", f"{beta:.3f}", x.shape[0], loss, f"{share:.3f}",
                     *learner_alone(learner(), a.envs, a.eval_steps, SEED + 1)))
    if device_fit:
        policy.close()
    env.close()
    print(f"{a.envs} envs; {a.steps} steps per rollout; {a.fit_steps} Adam steps per fit ({a.fit}); learner alone: {a.eval_steps} steps")
    print(f"expert alone over {a.steps} steps: {expert[0]} successes, {expert[1]} placed of {expert[2]} episodes ended")
    print("| stage | beta | pairs | last loss | expert acted | learner alone: successes | placed | episodes ended | success rate |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, beta, pairs, ls, share, ok, placed, ended in rows:
        rate = f"{ok / ended:.3f}" if ended else "-"
        print(f"| {name} | {beta} | {pairs} | {ls:.3g} | {share} | {ok} | {placed} | {ended} | {rate} |")


if __name__ == "__main__":
    main()
