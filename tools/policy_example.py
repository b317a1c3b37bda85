"""Behaviour-clone the on-device expert into an MLP and evaluate it closed-loop, all on the device (an example,
not a benchmark and not a criterion: nobody has measured what success rate such a policy reaches).

  1. record expert (observation, action) pairs: rollout(n_steps=..., record=("obs", "target", "done")); the
     expert's abs_pos action of step t is the recorded target, its input the observation the env held before
     the step (the reset observation, then the record's previous slice: after an autoreset the new episode's);
  2. fit a two-hidden-layer tanh MLP (85 -> 256 -> 256 -> 4) with torch, a few hundred Adam steps on the
     normalised observations;
  3. MlpPolicy.from_torch(...).bind(env); env.rollout_policy(policy, n_steps): the env's own waves evaluate the
     network between two env steps of a fused launch;
  4. print the episodes that ended in success beside the expert's over the same number of steps.

  python tools/policy_example.py [--envs 1024] [--steps 300] [--fit-steps 300]
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from mujoco_manip_amd import _lib  # noqa: E402

SEED = 42
CFG = dict(tasks="all", action_mode="abs_pos", reward_type="staged", randomize_objects=True, autoreset=True, image_size=0)


def make_env(n, seed=SEED, lib=None):
    from mujoco_manip_amd.vec_env import PickPlaceVecEnv

    env = PickPlaceVecEnv(n, **CFG, lib=lib)
    env.reset(seed=[_lib.episode_seed(seed, i) for i in range(n)])
    return env


def expert_pairs(env, n_steps):
    """(inputs [T * N, 85], actions [T * N, 4]) of n_steps expert steps from the env's current state."""
    obs0 = env._obs.clone()
    rec = env.rollout(n_steps=n_steps, record=("obs", "target", "done"))
    inputs = torch.cat([obs0[None], rec["obs"][:-1]])
    return inputs.reshape(-1, _lib.NOBS), rec["target"].reshape(-1, 4)


def fit(inputs, actions, hidden=(256, 256), steps=300, batch=8192, lr=1e-3, seed=0):
    """An MLP fitted to (inputs, actions) by mean-squared error -> (net, obs_shift, obs_scale): the network reads
    (obs - obs_shift) * obs_scale, the observation standardised per entry (constant entries dropped)."""
    nn = torch.nn
    gen = torch.Generator(device=inputs.device).manual_seed(seed)
    torch.manual_seed(seed)
    shift, sd = inputs.mean(0), inputs.std(0)
    scale = torch.where(sd > 1e-6, 1.0 / sd.clamp_min(1e-6), torch.zeros_like(sd))
    x = (inputs - shift) * scale
    mods, n_in = [], _lib.NOBS
    for w in hidden:
        mods += [nn.Linear(n_in, w), nn.Tanh()]
        n_in = w
    net = nn.Sequential(*mods, nn.Linear(n_in, actions.shape[1])).to(inputs.device)
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    for _ in range(steps):
        idx = torch.randint(0, x.shape[0], (min(batch, x.shape[0]),), device=x.device, generator=gen)
        loss = ((net(x[idx]) - actions[idx]) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    return net, shift, scale, float(loss.item())


def cloned_policy(n_envs=1024, record_steps=300, fit_steps=300, seed=SEED):
    """The example's policy, as (net, obs_shift, obs_scale, last loss)."""
    env = make_env(n_envs, seed)
    inputs, actions = expert_pairs(env, record_steps)
    out = fit(inputs, actions, steps=fit_steps)
    env.synchronize()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--fit-steps", type=int, default=300)
    a = ap.parse_args()
    from mujoco_manip_amd.policy import MlpPolicy

    ok = _lib.EPI["successes"]
    env = make_env(a.envs)
    inputs, actions = expert_pairs(env, a.steps)
    env.synchronize()
    expert = (int(env._epi[:, ok].sum()), int(env._epi[:, _lib.EPI["episodes"]].sum()))
    env.close()
    net, shift, scale, loss = fit(inputs, actions, steps=a.fit_steps)
    env = make_env(a.envs)
    ep0 = int(env._epi[:, _lib.EPI["episodes"]].sum())
    policy = MlpPolicy.from_torch(net, obs_shift=shift, obs_scale=scale).bind(env)
    out = env.rollout_policy(policy, a.steps, record=("done",))
    env.synchronize()
    cloned = (int(env._epi[:, ok].sum()), int(env._epi[:, _lib.EPI["episodes"]].sum()) - ep0)
    # the device's network against torch's own forward pass on the first observations
    x = inputs[:256]
    with torch.no_grad():
        gap = float((policy.eval(x) - net((x - shift) * scale)).abs().max())
    policy.close()
    env.close()
    print(f"{a.envs} envs x {a.steps} steps; fit: {a.fit_steps} Adam steps on {inputs.shape[0]} pairs, last loss {loss:.3g}")
    print(f"expert: {expert[0]} successful episodes; cloned policy: {cloned[0]} ({cloned[1]} episodes ended, "
          f"{int(out['done'][:, :, 2].sum())} success flags in the record); max |device - torch| on 256 rows = {gap:.2e}")


if __name__ == "__main__":
    main()
