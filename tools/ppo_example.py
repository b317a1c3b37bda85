"""PPO on the device (an example, not a benchmark and not a criterion: it is run by no test and carries no gate;
CHANGELOG.md holds the table of one run, whatever it showed).

Every iteration, with the observations, actions and weights staying on the device:
  1. env.rollout_policy(actor, steps, record = obs, reward, done, mean, noise): the actor (a Gaussian MlpPolicy) drives
     the envs inside the fused step launches;
  2. the observation each step was given = the env's observation before the call, then the record's previous slice
     (after an autoreset the new episode's first);
  3. critic.eval on them and on the observation after the last step -> env.gae(reward, done, value, value_last,
     normalize=True): advantages and returns;
  4. actor.fit_pg(obs, mean, noise, adv, ...): minibatch Adam steps of PPO's clipped surrogate, in place in the actor's
     device weights; critic.fit(obs, ret, ...): the value regression with the MSE fit;
  5. actor.set_log_std: a linear schedule from --log-std0 to --log-std1.
Printed per iteration: the mean reward per step and the mean return of the record's steps, the last step's three
statistics (surrogate loss, approximate KL, clipped fraction) and the critic's last loss.

--init dagger starts from an actor cloned from the on-device expert (tools/policy_example.cloned_policy); --init
random (the default) from small random weights.

  python tools/ppo_example.py [--envs 256] [--steps 64] [--iters 10] [--init random|dagger] [--fit-steps 20]
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]
from mujoco_manip_amd import _lib  # noqa: E402
from policy_example import SEED, cloned_policy, make_env  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=64, help="env steps per rollout")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--init", choices=("random", "dagger"), default="random")
    ap.add_argument("--fit-steps", type=int, default=20, help="optimisation steps of actor and critic per iteration")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--log-std0", type=float, default=-2.0)
    ap.add_argument("--log-std1", type=float, default=-3.0)
    a = ap.parse_args()
    from mujoco_manip_amd.policy import MlpCritic, MlpPolicy

    if not torch.cuda.is_available():
        raise SystemExit("ppo_example.py runs on the GPU: none found")
    nn = torch.nn
    env = make_env(a.envs, SEED)
    dev = env.device
    log_std = torch.full((4,), a.log_std0)
    if a.init == "dagger":
        net, shift, scale, _ = cloned_policy(n_envs=a.envs)
    else:
        torch.manual_seed(0)
        obs0 = env._obs.clone()
        shift, sd = obs0.mean(0), obs0.std(0)
        scale = torch.where(sd > 1e-6, 1.0 / sd.clamp_min(1e-6), torch.zeros_like(sd))
        net = nn.Sequential(nn.Linear(85, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
        with torch.no_grad():  # start at the middle of the action box
            from mujoco_manip_amd.planner import action_box

            low, high = (torch.tensor(v, device=dev) for v in action_box("abs_pos"))
            net[-1].weight.mul_(0.01)
            net[-1].bias.copy_(0.5 * (low + high))
    torch.manual_seed(1)
    vnet = nn.Sequential(nn.Linear(85, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)
    actor = MlpPolicy.from_torch(net, obs_shift=shift, obs_scale=scale, log_std=log_std, seed=SEED).bind(env)
    critic = MlpCritic.from_torch(vnet, obs_shift=shift, obs_scale=scale).bind(env)
    T, N = a.steps, a.envs
    print(f"PPO example: {N} envs x {T} steps per iteration, {a.fit_steps} steps of batch {a.batch}, init {a.init}")
    print("iter  reward/step  mean return  surrogate   approx KL  clipped  critic loss  log_std")
    for it in range(a.iters):
        first = env._obs.clone()
        rec = env.rollout_policy(actor, T, record=("obs", "reward", "done", "mean", "noise"), call=it)
        obs = torch.cat([first[None], rec["obs"][:-1]]).reshape(-1, _lib.NOBS).contiguous()
        value = critic.eval(obs).reshape(T, N)
        value_last = critic.eval(rec["obs"][-1])[:, 0].contiguous()
        adv, ret = env.gae(rec["reward"], rec["done"], value, value_last, gamma=a.gamma, lam=a.lam, normalize=True)
        stats = actor.fit_pg(obs, rec["mean"].reshape(-1, 4), rec["noise"].reshape(-1, 4), adv.reshape(-1), a.fit_steps, clip=a.clip,
                             batch=a.batch, lr=a.lr, seed=it)
        closs = critic.fit(obs, ret.reshape(-1, 1), a.fit_steps, batch=a.batch, lr=1e-3, seed=it)
        ls = a.log_std0 + (a.log_std1 - a.log_std0) * (it + 1) / a.iters
        actor.set_log_std(torch.full((4,), ls))
        s = stats[-1].tolist()
        print(f"{it:4d}  {rec['reward'].mean().item():11.4f}  {ret.mean().item():11.4f}  {s[0]:9.4f}  {s[1]:10.3e}  {s[2]:7.3f}"
              f"  {closs[-1].item():11.4f}  {ls:7.3f}")
    env.synchronize()
    for p in (actor, critic):
        p.close()
    env.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
