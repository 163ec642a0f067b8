"""skrl 1.1 ``PPO._update`` and ``record_transition`` as rover_ppo.yaml configures them: the CPU-capable specification of the gated
fused update (``include/rover_train_gate.h``, ``ppo.FusedPPO.update(kl_early_stop=..., scheduler=...)``) and of the shaped record
launch (``rover_rollout_record_shaped``).

rover_ppo.yaml (and rover_rpo.yaml) set ``kl_threshold: 0.008`` and leave ``learning_rate_scheduler`` commented out.  In skrl 1.1
``kl_threshold`` is the KL EARLY STOP::

    for epoch in range(learning_epochs):
        kl_divergences = []
        for minibatch in sampled_batches:
            sampled_states = state_preprocessor(sampled_states, train=not epoch)
            ... kl_divergence = ((ratio - 1) - log ratio).mean();  kl_divergences.append(kl_divergence)
            if kl_threshold and kl_divergence > kl_threshold: break        # before backward() and optimizer.step()
            ... backward, clip_grad_norm_, optimizer.step()
        if learning_rate_scheduler: scheduler.step(mean(kl_divergences))      # KLAdaptiveRL

``examples/04_train_ppo.py`` (and so ``ppo_scaled.TorchScaledPPO``) reads ``kl_threshold`` as KLAdaptiveRL's threshold and never
stops an epoch; ``TorchSkrlPPO`` with ``kl_early_stop=0`` and ``scheduler="kl_adaptive"`` is exactly that update.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .lift_ppo import kl_adaptive
from .ppo_scaled import TorchScaledPPO, ppo_loss


def shape_rewards(rew: torch.Tensor, val: torch.Tensor, truncated: torch.Tensor, scale: float = 1.0, discount: float = 0.99,
                  time_limit_bootstrap: bool = False) -> torch.Tensor:
    """skrl ``PPO.record_transition`` on the rewards: the reference's ``reward_shaper_function`` (``rewards * scale``,
    rover_envs/utils/config.py:84-88), then with ``time_limit_bootstrap`` ``rewards += discount_factor * values * truncated``
    (``values``: the critic on the pre-step states, on the return's scale).  A new tensor; the inputs are not written."""
    r = rew * scale
    if time_limit_bootstrap:
        r += discount * val * truncated
    return r


class TorchSkrlPPO(TorchScaledPPO):
    """The spec: skrl's update loops on ``Net`` modules with ``torch.optim.Adam``.  ``scalers=False``: no preprocessors (the
    states reach the networks as they are; ``standardize_values`` is the identity)."""

    def __init__(self, policy: nn.Module, value: nn.Module, lr: float = 1e-4, epochs: int = 4, minibatches: int = 60,
                 max_grad_norm: float = 0.5, scalers: bool = True, device="cuda"):
        super().__init__(policy, value, lr=lr, epochs=epochs, minibatches=minibatches, max_grad_norm=max_grad_norm, device=device)
        if not scalers:
            self.state_preprocessor = self.value_preprocessor = None
        self.steps = 0                 # optimiser steps taken
        self.last_update = None        # per-epoch {"recorded", "stopped"} of the last update
        self.last_kls = None           # the recorded minibatch KLs of the last update, per epoch

    @torch.no_grad()
    def standardize_values(self, val: torch.Tensor, ret: torch.Tensor):
        if self.value_preprocessor is None:
            return val, ret
        return super().standardize_values(val, ret)

    def update(self, obs, act, logp, val, ret, adv, perms=None, epochs: int | None = None, minibatches: int | None = None,
               train_state_scaler: bool = True, kl_early_stop: float = 0.0, scheduler: str | None = "kl_adaptive"):
        """As ``TorchScaledPPO.update``; ``kl_early_stop`` > 0 stops an epoch at the first minibatch whose KL exceeds it, before
        its optimiser step (the KL is recorded); ``scheduler``: None or "kl_adaptive", stepped per epoch on the mean of the
        recorded KLs.  Returns (epoch KL means, learning rate)."""
        if scheduler not in (None, "kl_adaptive"):
            raise ValueError('scheduler must be None or "kl_adaptive"')
        epochs = self.epochs if epochs is None else int(epochs)
        mbs = self.minibatches if minibatches is None else int(minibatches)
        obs = obs.reshape(-1, obs.shape[-1])
        B = obs.shape[0]
        act = act.reshape(B, -1)
        logp, val, ret, adv = (x.reshape(B) for x in (logp, val, ret, adv))
        params = list(self.policy.parameters()) + list(self.value.parameters())
        kls_out, recorded, stopped, all_kls = [], [], [], []
        for epoch in range(epochs):
            perm = perms[epoch] if perms is not None else torch.randperm(B, device=self.device)
            kls, stop = [], False
            for mb in perm.chunk(mbs):
                s = obs[mb]
                if self.state_preprocessor is not None:
                    with torch.no_grad():
                        s = self.state_preprocessor(s, train=train_state_scaler and not epoch)
                loss, kl = ppo_loss(self.policy, self.value, s, act[mb], logp[mb], val[mb], ret[mb], adv[mb])
                kls.append(kl)
                if kl_early_stop and kl > kl_early_stop:
                    stop = True
                    break
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                nn.utils.clip_grad_norm_(params, self.max_grad_norm)
                self.opt.step()
                self.steps += 1
            kl_mean = torch.stack(kls).mean().item()
            kls_out.append(kl_mean)
            recorded.append(len(kls)); stopped.append(stop); all_kls.append([float(k) for k in kls])
            if scheduler is not None:
                lr = kl_adaptive(self.lr, kl_mean)
                for g in self.opt.param_groups:
                    g["lr"] = lr
        self.last_update = {"recorded": recorded, "stopped": stopped}
        self.last_kls = all_kls
        return kls_out, self.lr

    def state_dict(self) -> dict:
        if self.state_preprocessor is None:
            return {"policy": self.policy.state_dict(), "value": self.value.state_dict()}
        return super().state_dict()

