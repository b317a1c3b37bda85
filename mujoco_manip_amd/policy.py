"""MlpPolicy — a learned policy a_t = pi(obs_t) evaluated inside the fused step launches (mmx_rollout_policy,
include/mmx_api.h): the env's own wave runs the network between two env steps, so a closed-loop rollout makes
no launch, and no host round trip, per env step.

The network is a multi-layer perceptron on the flat numeric observation [85] (vec_env.split_obs names its
slices): x = (obs - obs_shift) * obs_scale, up to four linear layers of at most 256 outputs with tanh or ReLU
between them, and action = clip(mean + exp(log_std) * z, low, high) with z a counter-based normal draw that
depends on (seed, call, step, env, component) alone (log_std None: deterministic).

    policy = MlpPolicy.from_torch(net, obs_shift=mu, obs_scale=1 / sd)     # net: nn.Sequential(Linear, Tanh, ...)
    policy.bind(env)
    out = env.rollout_policy(policy, n_steps=100)          # {"obs", "reward", "done", "actions"}: [T, N, ...]
    mean = policy.eval(dataset_obs)                        # the network alone, for behaviour-cloning validation
    policy.close()                                         # before env.close()

This module imports without a GPU; bind() needs one.
"""
from __future__ import annotations

import numpy as np

from . import _lib

ACTIVATIONS = _lib.POLICY_ACTIVATIONS


def _f32(a, name: str, shape=None):
    """A float32 numpy copy of a numpy array, a torch tensor or a sequence; `shape`: the shape it must have."""
    if a is None:
        return None
    if hasattr(a, "detach"):  # a torch tensor, on any device
        a = a.detach().cpu().numpy()
    a = np.array(a, dtype=np.float32)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {a.shape}")
    return np.ascontiguousarray(a)


def _fit_config(steps, batch, lr, betas, eps, optimizer, shuffle, seed, reset_optimizer):
    """(steps, mmx_fit_config) of fit's and fit_pg's common arguments, validated."""
    if optimizer not in _lib.FIT_OPTIMIZERS:
        raise ValueError(f"optimizer must be one of {_lib.FIT_OPTIMIZERS}, got '{optimizer}'")
    steps, batch = int(steps), int(batch)
    if steps < 0:
        raise ValueError(f"steps must be >= 0, got {steps}")
    if not 1 <= batch <= _lib.FIT_MAX_BATCH:
        raise ValueError(f"batch must be in 1 .. {_lib.FIT_MAX_BATCH}, got {batch}")
    b1, b2 = (float(v) for v in betas)
    if not (np.isfinite(lr) and lr > 0 and np.isfinite(eps) and eps > 0 and 0 <= b1 < 1 and 0 <= b2 < 1):
        raise ValueError("lr and eps must be finite and > 0, betas in [0, 1)")
    return steps, _lib.MMXFitConfig(optimizer=_lib.FIT_OPTIMIZERS.index(optimizer), batch=batch, shuffle=int(bool(shuffle)),
                                    reset_optimizer=int(bool(reset_optimizer)), lr=lr, beta1=b1, beta2=b2, eps=eps,
                                    seed=int(seed) & (2**64 - 1))


def _check_rows(env, tensors) -> int:
    """n, given that every (name, tensor, width) is a contiguous float32 torch tensor [n, width] ([n] at width 0) on
    the env's device with the same n in 1 .. 2^31 - 1."""
    import torch

    for name, t, width in tensors:
        shape = f"[n, {width}]" if width else "[n]"
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor on {env.device}")
        if t.dtype != torch.float32 or t.dim() != (2 if width else 1) or (width and t.shape[1] != width):
            raise ValueError(f"{name} must be float32 {shape}, got {t.dtype} {tuple(t.shape)}")
        if t.device != torch.device(env.device):
            raise ValueError(f"{name} must be on {env.device}, got {t.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    rows = [t.shape[0] for _, t, _ in tensors]
    if len(set(rows)) != 1 or not 1 <= rows[0] < 2**31:
        raise ValueError(f"{', '.join(n for n, _, _ in tensors)} must have the same number of rows in 1 .. 2^31 - 1, got {rows}")
    return rows[0]


class MlpPolicy:
    def __init__(self, layers, activation: str = "tanh", obs_shift=None, obs_scale=None, log_std=None, low=None,
                 high=None, seed: int = 0):
        """layers: [(W [out, in], b [out] or None), ...], W as torch.nn.Linear.weight; the first layer reads the 85
        observation entries, the last one's outputs are the action.  low / high None: the action mode's box
        (planner.action_box) once bound, where it has one."""
        layers = list(layers)
        if not 1 <= len(layers) <= _lib.POLICY_MAX_LAYERS:
            raise ValueError(f"a policy has 1 to {_lib.POLICY_MAX_LAYERS} linear layers, got {len(layers)}")
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation must be one of {ACTIVATIONS}, got '{activation}'")
        self.layers, n_in = [], _lib.NOBS
        for k, layer in enumerate(layers):
            W, b = layer if isinstance(layer, (tuple, list)) else (layer, None)
            W = _f32(W, f"layers[{k}] weight")
            if W.ndim != 2 or W.shape[1] != n_in:
                raise ValueError(f"layers[{k}] weight must be [out, {n_in}], got {W.shape}")
            if not 1 <= W.shape[0] <= _lib.POLICY_MAX_WIDTH:
                raise ValueError(f"layers[{k}] has {W.shape[0]} outputs; a layer has 1 to {_lib.POLICY_MAX_WIDTH}")
            self.layers.append((W, _f32(b, f"layers[{k}] bias", (W.shape[0],))))
            n_in = W.shape[0]
        self.action_dim = n_in
        if self.action_dim > _lib.MPPI_MAX_ADIM:
            raise ValueError(f"the last layer has {self.action_dim} outputs; an action has at most {_lib.MPPI_MAX_ADIM}")
        self.activation = activation
        self.obs_shift = _f32(obs_shift, "obs_shift", (_lib.NOBS,))
        self.obs_scale = _f32(obs_scale, "obs_scale", (_lib.NOBS,))
        self.log_std = _f32(log_std, "log_std", (self.action_dim,))
        self.low = _f32(low, "low", (self.action_dim,))
        self.high = _f32(high, "high", (self.action_dim,))
        self.seed = int(seed)
        self._dev = None
        self._env = None

    @classmethod
    def from_torch(cls, net, **kw) -> "MlpPolicy":
        """From a torch.nn.Sequential of Linear layers with Tanh or ReLU modules (all the same) between them."""
        import torch.nn as nn

        mods = list(net)
        if not mods or len(mods) % 2 == 0:
            raise ValueError("from_torch needs Linear layers with one activation module between each pair")
        lin, acts = mods[0::2], mods[1::2]
        if not all(isinstance(m, nn.Linear) for m in lin):
            raise ValueError("from_torch: every other module, from the first, must be a torch.nn.Linear")
        kinds = {type(m) for m in acts}
        if not kinds <= {nn.Tanh, nn.ReLU} or len(kinds) > 1:
            raise ValueError("from_torch: the modules between the Linear layers must be all Tanh or all ReLU")
        activation = "relu" if kinds == {nn.ReLU} else "tanh"
        return cls([(m.weight, m.bias) for m in lin], activation=activation, **kw)

    # ------------------------------------------------------------------ the device object
    def bind(self, env) -> "MlpPolicy":
        """Create the device object on the env's device (a PickPlaceVecEnv whose action dimension is the last
        layer's width); a policy bound before is closed first."""
        if env.action_dim != self.action_dim:
            raise ValueError(f"the policy's last layer has {self.action_dim} outputs, the env's action_dim is {env.action_dim}")
        self.close()
        low, high = self.low, self.high
        if low is None or high is None:
            from .planner import action_box

            box_low, box_high = action_box(env._action_mode)
            low = np.asarray(box_low, np.float32) if low is None else low
            high = np.asarray(box_high, np.float32) if high is None else high
        self._dev = _lib.Policy(env.sim, self.layers, ACTIVATIONS.index(self.activation), self.obs_shift, self.obs_scale,
                                self.log_std, low, high, self.seed)
        self._env = env
        self.bound_low, self.bound_high = low, high
        return self

    @property
    def device_policy(self) -> "_lib.Policy":
        if self._dev is None:
            raise RuntimeError("the policy is not bound: call bind(env) first")
        return self._dev

    def eval(self, obs):
        """The network alone: mean [n, A] (a CUDA tensor) of observations [n, 85], no noise, no clamp."""
        import torch

        dev, env = self.device_policy, self._env
        x = torch.as_tensor(obs, dtype=torch.float32, device=env.device)
        if x.dim() != 2 or x.shape[1] != _lib.NOBS:
            raise ValueError(f"obs must be [n, {_lib.NOBS}], got {tuple(x.shape)}")
        x = x.contiguous()
        out = torch.empty((x.shape[0], self.action_dim), dtype=torch.float32, device=env.device)
        if x.shape[0]:
            with env.sim._on_sim_stream(env.device) as (cur, sst):
                x.record_stream(sst)
                out.record_stream(sst)
                dev.eval(x.data_ptr(), x.shape[0], out.data_ptr())
        return out

    # ------------------------------------------------------------------ fitting on the device (mmx_policy_fit)
    def fit(self, obs, target, steps: int, batch: int = 8192, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
            optimizer: str = "adam", shuffle: bool = True, seed: int = 0, reset_optimizer: bool = False):
        """`steps` minibatch gradient steps of the mean-squared error between the network's output and `target` on
        the pairs (obs [n, 85], target [n, A]: contiguous float32 torch tensors on the policy's device), which
        update the bound policy's weights in place on the env's stream: the next rollout or eval runs them.
        Returns the losses [steps] (a device tensor; loss[i] is the batch loss before update i).  The optimiser's
        moments and step count persist across calls unless reset_optimizer.  self.layers keeps the weights the
        policy was made with until weights() refreshes it."""
        import torch

        dev, env = self.device_policy, self._env
        steps, cfg = _fit_config(steps, batch, lr, betas, eps, optimizer, shuffle, seed, reset_optimizer)
        n = _check_rows(env, (("obs", obs, _lib.NOBS), ("target", target, self.action_dim)))
        loss = torch.empty(steps, dtype=torch.float32, device=env.device)
        if steps:
            with env.sim._on_sim_stream(env.device) as (cur, sst):
                for t in (obs, target, loss):
                    t.record_stream(sst)
                dev.fit(obs.data_ptr(), target.data_ptr(), n, steps, cfg, loss.data_ptr())
        return loss

    # ------------------------------------------------------------------ policy gradients (mmx_policy_fit_pg)
    def fit_pg(self, obs, mean_old, noise, adv, steps: int, clip: float = 0.2, batch: int = 8192, lr: float = 3e-4,
               betas=(0.9, 0.999), eps: float = 1e-8, optimizer: str = "adam", shuffle: bool = True, seed: int = 0,
               reset_optimizer: bool = False):
        """`steps` minibatch steps of PPO's clipped surrogate -mean(min(r adv, clip(r, 1 - clip, 1 + clip) adv)) on
        the samples of a rollout: obs [n, 85] (what each step was given), mean_old and noise [n, A] (the rollout's
        record of that name), adv [n] (PickPlaceVecEnv.gae); contiguous float32 torch tensors on the policy's
        device.  r is the ratio of the policy's density now to the one at the rollout, of the sample before the
        clamp; log_std is not trained (set_log_std schedules it).  Updates the weights in place on the env's stream
        like fit, with which it shares the optimiser's moments and step count.  Returns the statistics [steps, 3]
        (a device tensor): per step, before its update, the surrogate loss, the approximate KL mean((r - 1) - log r)
        and the fraction of samples the clip removed from the gradient."""
        import torch

        dev, env = self.device_policy, self._env
        steps, cfg = _fit_config(steps, batch, lr, betas, eps, optimizer, shuffle, seed, reset_optimizer)
        n = _check_rows(env, (("obs", obs, _lib.NOBS), ("mean_old", mean_old, self.action_dim), ("noise", noise, self.action_dim),
                              ("adv", adv, 0)))
        if not (np.isfinite(clip) and 0 < clip < 1):
            raise ValueError(f"clip must be in (0, 1), got {clip}")
        if self.log_std is None:
            raise ValueError("fit_pg needs a stochastic policy (log_std): a deterministic one has no likelihood ratio")
        stats = torch.empty((steps, 3), dtype=torch.float32, device=env.device)
        if steps:
            with env.sim._on_sim_stream(env.device) as (cur, sst):
                for t in (obs, mean_old, noise, adv, stats):
                    t.record_stream(sst)
                dev.fit_pg(obs.data_ptr(), mean_old.data_ptr(), noise.data_ptr(), adv.data_ptr(), n, steps,
                           _lib.MMXPgConfig(fit=cfg, clip=float(clip)), stats.data_ptr())
        return stats

    def set_log_std(self, log_std):
        """Sets the bound policy's log_std [A] in place (waits for the env's stream); the next rollout draws
        its actions with exp(log_std).  Nothing else of the policy changes."""
        dev = self.device_policy
        log_std = _f32(log_std, "log_std", (self.action_dim,))
        if not np.isfinite(log_std).all():
            raise ValueError("log_std must be finite")
        dev.set_log_std(log_std)
        self.log_std = log_std

    def weights(self):
        """[(W [out, in], b [out]), ...] numpy arrays (torch layout) of the bound policy's weights as they are now;
        self.layers becomes this list.  Waits for the env's stream."""
        self.layers = self.device_policy.get_weights()
        return self.layers

    def to_torch(self, net):
        """Copies the bound policy's current weights into `net`, a torch.nn.Sequential of the shape from_torch
        takes (a Linear without a bias must belong to a layer whose bias is 0: it cannot hold one)."""
        import torch

        layers = self.weights()
        lin = list(net)[0::2]
        if len(lin) != len(layers) or any(tuple(m.weight.shape) != W.shape for m, (W, _) in zip(lin, layers)):
            raise ValueError("to_torch: the net's Linear layers do not match the policy's")
        with torch.no_grad():
            for m, (W, b) in zip(lin, layers):
                m.weight.copy_(torch.from_numpy(W))
                if m.bias is not None:
                    m.bias.copy_(torch.from_numpy(b))
                elif np.any(b != 0):
                    raise ValueError("to_torch: a Linear without a bias cannot take a layer whose bias is not 0")
        return net

    def load(self, net_or_layers):
        """Sets the bound policy's weights in place from a torch.nn.Sequential (as from_torch) or from a list
        [(W, b or None), ...] of the policy's own shapes; the optimiser's state stays."""
        dev = self.device_policy
        if hasattr(net_or_layers, "parameters"):
            src = MlpPolicy.from_torch(net_or_layers)
            if src.activation != self.activation and len(src.layers) > 1:
                raise ValueError(f"load: the net's activation is {src.activation}, the policy's {self.activation}")
            layers = src.layers
        else:
            layers = [(_f32(W, "weight"), _f32(b, "bias")) for W, b in net_or_layers]
        dev.set_weights(layers)
        self.layers = [(W, b) for W, b in layers]

    def close(self):
        if self._dev is not None:
            self._dev.close()
        self._dev = self._env = None


class MlpCritic(MlpPolicy):
    """A value network V(obs): an MlpPolicy whose last layer has width 1, with no log_std and no action box.  eval
    gives V [n, 1] and fit regresses it to targets [n, 1] (PickPlaceVecEnv.gae's returns); it is never rolled out.

        critic = MlpCritic.from_torch(vnet, obs_shift=mu, obs_scale=1 / sd).bind(env)
        value = critic.eval(obs.reshape(-1, 85)).reshape(T, N)
        adv, ret = env.gae(rec["reward"], rec["done"], value, critic.eval(env_obs)[:, 0])
        critic.fit(obs.reshape(-1, 85), ret.reshape(-1, 1), steps=10)
    """

    def __init__(self, layers, activation: str = "tanh", obs_shift=None, obs_scale=None, seed: int = 0):
        super().__init__(layers, activation=activation, obs_shift=obs_shift, obs_scale=obs_scale, seed=seed)
        if self.action_dim != 1:
            raise ValueError(f"a critic's last layer has 1 output, got {self.action_dim}")

    def bind(self, env) -> "MlpCritic":
        """Create the device object on the env's device, whatever the env's action dimension: no box, no clamp."""
        self.close()
        self._dev = _lib.Policy(env.sim, self.layers, ACTIVATIONS.index(self.activation), self.obs_shift, self.obs_scale,
                                None, None, None, self.seed)
        self._env = env
        return self

    def fit_pg(self, *args, **kw):
        raise TypeError("a critic has no policy gradient: fit it on the returns with fit()")

    def set_log_std(self, log_std):
        raise TypeError("a critic has no log_std")
