"""The rollout collector behind skrl's running scalers (``state_preprocessor`` / ``value_preprocessor``): ``rollout.RolloutCollector``'s
interface and buffers, with the networks reading STANDARDISED rows and the stored values back on the original scale.

skrl's PPO (``act`` / ``record_transition``) keeps the raw states in memory, feeds ``state_preprocessor(states)`` to both models
and stores ``value_preprocessor(values, inverse=True)``.  ``ScaledRolloutCollector.act`` is three launches:

    1. ``rover_scaler_apply`` with sanitise: the raw rows -> ``obs[t]`` (sanitised) and an (n, 965) scratch (standardised);
    2. the unchanged ``rover_rollout_act`` on the scratch (its own ``nan_to_num`` is the identity on clamped finite rows);
    3. ``rover_scaler_apply`` in inverse mode, width 1: the critic's outputs -> ``val[t]``.

``record`` is ``RolloutCollector``'s, ``rewards_shaper_scale`` / ``time_limit_bootstrap`` included: slot ``t`` of ``val`` is on the
original scale, the return's, as skrl's bootstrap wants it.

Both scalers are ``scaler.DeviceScaler`` s held BY REFERENCE (``FusedScaledPPO.state_scaler`` / ``.value_scaler``): an update of
the trainer's is seen by the next step.  ``TorchScaledRollout`` is the CPU specification on ``rollout.TorchRollout``.
"""
from __future__ import annotations

import torch

from .rollout import RolloutCollector, TorchRollout, rollout_act
from .scaler import DeviceScaler


class TorchScaledRollout(TorchRollout):
    """The specification.  ``state_scaler`` / ``value_scaler``: ``lift_ppo.RunningStandardScaler`` s (any callables with its
    ``(x, inverse=False)`` signature); ``actor`` / ``critic`` read standardised rows."""

    def __init__(self, actor, critic, log_std, state_scaler, value_scaler, num_envs: int, horizon: int, **kw):
        super().__init__(None, None, log_std, num_envs, horizon, **kw)
        self.nets = (actor, critic)
        self.state_scaler, self.value_scaler = state_scaler, value_scaler
        # what TorchRollout calls on the sanitised rows
        self.actor = lambda o: self.nets[0](self.state_scaler(o))
        self.critic = lambda o: self.value_scaler(self.nets[1](self.state_scaler(o)).reshape(-1, 1), inverse=True)


class ScaledRolloutCollector(RolloutCollector):
    """The fused rollout behind the scalers: ``actor`` / ``critic`` / ``log_std`` as ``RolloutCollector`` takes them (with
    ``FusedScaledPPO.actor`` / ``.critic`` / ``.log_std`` always the trainer's current parameters).  ``val_s`` holds the critic's
    outputs of the last call before the inverse transform, ``states`` the standardised rows."""

    def __init__(self, actor, critic, log_std: torch.Tensor, state_scaler: DeviceScaler, value_scaler: DeviceScaler, num_envs: int,
                 horizon: int, **kw):
        super().__init__(actor, critic, log_std, num_envs, horizon, **kw)
        if state_scaler.width != 965 or value_scaler.width != 1:
            raise ValueError("state_scaler must have 965 columns and value_scaler 1")
        if state_scaler.block.device != self.obs.device or value_scaler.block.device != self.obs.device:
            raise ValueError(f"the scalers must live on {self.device}")
        self.state_scaler, self.value_scaler = state_scaler, value_scaler
        self.states = torch.zeros(self.n, 965, dtype=torch.float32, device=self.device)
        self.val_s = torch.zeros(self.n, 1, dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def act(self, t: int, raw_obs) -> torch.Tensor:
        raw = self._raw(raw_obs)
        self.state_scaler.forward(raw, out=self.states, sanitise=True, raw_out=self.obs[t])
        rollout_act(self.actor, self.critic, self.log_std, self.states, self.counter, self.hparams(), mean_out=self.mean[t],
                    val_out=self.val_s, act_out=self.actions[t], env_act_out=self._env_act, logp_out=self.logp[t])
        self.value_scaler.inverse(self.val_s, out=self.val[t])
        self.counter += 1
        return self._env_act

    @torch.no_grad()
    def last_value(self, raw_obs) -> torch.Tensor:
        """The bootstrap value of the rows after the last step, on the original scale: no draw, the counter stays."""
        self.state_scaler.forward(self._raw(raw_obs), out=self.states, sanitise=True)
        rollout_act(self.actor, self.critic, self.log_std, self.states, self.counter, self.hparams(), mean_out=self._last_mean,
                    val_out=self.val_s)
        self.value_scaler.inverse(self.val_s, out=self._last_val)
        return self._last_val[:, 0]
