"""DAgger (Ross et al. 2011) on the device: PickPlaceVecEnv.rollout_dagger rolls out an MlpPolicy, or a per-step
mixture of it and the FSM expert, inside the fused step launches and records at every visited state what the
expert would have done (mmx_rollout_dagger, include/mmx_api.h); DaggerBuffer aggregates the (observation, label)
pairs for the next fit.

    buf = DaggerBuffer(capacity=2_000_000)
    for k in range(rounds):
        policy = MlpPolicy.from_torch(net, obs_shift=mu, obs_scale=1 / sd).bind(env)
        rec = env.rollout_dagger(policy, 100, beta=0.5 ** k, call=k)      # {"obs_in", "expert_action", "gate", ...}
        buf.add(rec)
        obs, label = buf.tensors()                                        # [n, 85], [n, 4]: retrain net on them
        policy.close()

tools/dagger_example.py is the whole loop.  This module is plain torch and Python: the kernel is the rollout's.
"""
from __future__ import annotations

import math

from . import _lib

# what rollout_dagger records by default: the training pairs, who acted, and the trajectory's flags
DEFAULT_RECORD = ("obs_in", "expert_action", "gate", "reward", "done")


def check_args(n_steps, beta, takeover_dist, record):
    """The arguments of PickPlaceVecEnv.rollout_dagger, validated without a device -> (T, beta, takeover_dist,
    names): n_steps >= 0; beta a probability; takeover_dist >= 0 and finite (0: no takeover); record entries among
    _lib.TRAJ_FIELDS and _lib.DAGGER_FIELDS."""
    names = (record,) if isinstance(record, str) else tuple(record or ())
    allowed = tuple(_lib.TRAJ_FIELDS) + tuple(_lib.DAGGER_FIELDS)
    for name in names:
        if name not in allowed:
            raise ValueError(f"record entries must be among {allowed}, got '{name}'")
    if n_steps is None or isinstance(n_steps, bool) or int(n_steps) != n_steps or int(n_steps) < 0:
        raise ValueError(f"rollout_dagger needs an integer n_steps >= 0, got {n_steps!r}")
    beta, takeover_dist = float(beta), float(takeover_dist)
    if not (0.0 <= beta <= 1.0):  # (a NaN fails the test)
        raise ValueError(f"beta must be a probability in [0, 1], got {beta}")
    if not (takeover_dist >= 0.0 and math.isfinite(takeover_dist)):
        raise ValueError(f"takeover_dist must be >= 0 and finite (0: no takeover), got {takeover_dist}")
    return int(n_steps), beta, takeover_dist, names


class DaggerBuffer:
    """The aggregate of DAgger: (obs_in, expert_action) pairs of any number of rollouts, kept on the device the
    records are on.  add(rec) takes a rollout_dagger record (or any dict with "obs_in" [T, N, 85] and
    "expert_action" [T, N, 4]) and appends its T * N pairs in (t, i) order; tensors() returns the two stacked
    tensors, oldest pair first.  capacity (None: unbounded) keeps the newest `capacity` pairs: after every add the
    oldest ones beyond it are dropped, so the content depends on the sequence of adds alone."""

    def __init__(self, capacity: int | None = None):
        if capacity is not None and (isinstance(capacity, bool) or int(capacity) != capacity or int(capacity) <= 0):
            raise ValueError(f"capacity must be a positive integer or None, got {capacity!r}")
        self.capacity = None if capacity is None else int(capacity)
        self._obs = None
        self._label = None
        self.dropped = 0  # pairs dropped so far

    def __len__(self) -> int:
        return 0 if self._obs is None else int(self._obs.shape[0])

    def add(self, rec) -> int:
        """Append the pairs of `rec`; returns the number of pairs now held."""
        import torch

        if "obs_in" not in rec or "expert_action" not in rec:
            raise ValueError('add needs a record with "obs_in" and "expert_action" (rollout_dagger records both by default)')
        obs, label = rec["obs_in"], rec["expert_action"]
        if obs.dim() != 3 or label.dim() != 3 or obs.shape[:2] != label.shape[:2] or obs.shape[2] != _lib.NOBS or label.shape[2] != 4:
            raise ValueError(f"obs_in must be [T, N, {_lib.NOBS}] and expert_action [T, N, 4], got {tuple(obs.shape)} and "
                             f"{tuple(label.shape)}")
        obs, label = obs.reshape(-1, _lib.NOBS), label.reshape(-1, 4)
        if self._obs is not None:
            if obs.device != self._obs.device:
                raise ValueError(f"the buffer is on {self._obs.device}, the record on {obs.device}")
            obs, label = torch.cat([self._obs, obs]), torch.cat([self._label, label])
        over = 0 if self.capacity is None else max(0, int(obs.shape[0]) - self.capacity)
        self.dropped += over
        self._obs, self._label = obs[over:].clone(), label[over:].clone()
        return len(self)

    def tensors(self):
        """(obs [n, 85], expert_action [n, 4]), oldest first; None, None while empty."""
        return self._obs, self._label
