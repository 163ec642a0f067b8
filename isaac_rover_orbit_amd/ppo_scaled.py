"""Rover PPO with skrl's running state and value scalers (``state_preprocessor`` / ``value_preprocessor`` of rover_ppo.yaml).

``FusedScaledPPO`` composes an unchanged ``ppo.FusedPPO`` with two ``scaler.DeviceScaler`` s (965-wide states, 1-wide values) and
follows skrl 1.1 ``PPO._update`` as ``lift_ppo.TorchLiftPPO.update`` restates it: the state scaler trains on every minibatch of
the first epoch (``train=not epoch``) and only transforms afterwards.  The networks never see a gathered copy of the raw rows:
the trainer keeps ONE (B, 965) image of the rollout buffer, standardises a minibatch's rows into the same rows of the image
(``rover_scaler_apply`` with ``idx``), and hands the image with the same ``idx`` to ``FusedPPO.minibatch``.  After the first epoch
one pass rewrites the whole image with the final statistics, and the later epochs do no scaler work at all.

``TorchScaledPPO`` is the specification: the example's loss (examples/04_train_ppo.py) on ``Net`` modules, ``torch.optim.Adam``
and two ``lift_ppo.RunningStandardScaler`` s in the same order.

``update(kl_early_stop=0.008, scheduler=None)`` is skrl's KL early stop without a scheduler, rover_ppo.yaml as skrl reads it
(``include/rover_train_gate.h``; ``ppo_skrl.TorchSkrlPPO`` is its specification): the state scaler's training launches of the
first epoch sit behind the trainer's stop word (``rover_scaler_train_gated``), so the minibatch that stops the epoch still trains the
scaler and the skipped ones do not, as in skrl.  ``rewards_shaper_scale`` / ``time_limit_bootstrap`` are the collectors'
(``rollout.RolloutCollector.record``).  Not here: the entropy term at a non-zero scale (0 in the rover files).
"""
from __future__ import annotations

from typing import Mapping

import torch
import torch.nn as nn

from ._fused import load_checkpoint, require_gpu
from .lift_ppo import RunningStandardScaler, kl_adaptive
from .ppo import FusedPPO
from .scaler import DeviceScaler
from .trpo import log_prob

OBS_DIM = 965
STATE_KEY, VALUE_KEY = "state_preprocessor", "value_preprocessor"


def ppo_loss(policy, value, s, a, old_lp, old_v, ret, adv, clip=0.2, vclip=0.2):
    """examples/04_train_ppo.py ``ppo_loss`` on STANDARDISED states ``s``: (loss, kl)."""
    lp = log_prob(policy, s, a)
    ratio = (lp - old_lp).exp()
    with torch.no_grad():
        kl = ((ratio - 1) - (lp - old_lp)).mean()
    pl = -torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv).mean()
    v = value(s).squeeze(1)
    v = old_v + (v - old_v).clamp(-vclip, vclip)
    vl = ((ret - v) ** 2).mean()
    return pl + vl, kl


# ---------------------------------------------------------------------------------------------------------------- torch spec
class TorchScaledPPO:
    """The spec: the example's PPO update with skrl's two scalers, torch autograd and ``torch.optim.Adam``."""

    def __init__(self, policy: nn.Module, value: nn.Module, lr: float = 1e-4, epochs: int = 4, minibatches: int = 60,
                 max_grad_norm: float = 0.5, device="cuda"):
        self.device = torch.device(device)
        self.policy, self.value = policy.to(self.device), value.to(self.device)
        self.epochs, self.minibatches, self.max_grad_norm = int(epochs), int(minibatches), float(max_grad_norm)
        self.opt = torch.optim.Adam(list(self.policy.parameters()) + list(self.value.parameters()), lr=lr)
        self.state_preprocessor = RunningStandardScaler(OBS_DIM, device=self.device)
        self.value_preprocessor = RunningStandardScaler(1, device=self.device)

    @property
    def lr(self) -> float:
        return self.opt.param_groups[0]["lr"]

    @torch.no_grad()
    def standardize_values(self, val: torch.Tensor, ret: torch.Tensor):
        """skrl PPO._update: ``values = value_preprocessor(values, train=True)``, then the same on the returns."""
        v = self.value_preprocessor(val.reshape(-1, 1), train=True).reshape(val.shape)
        r = self.value_preprocessor(ret.reshape(-1, 1), train=True).reshape(ret.shape)
        return v, r

    def update(self, obs, act, logp, val, ret, adv, perms=None, epochs: int | None = None, minibatches: int | None = None,
               train_state_scaler: bool = True):
        """Flat (B, ...) or (T, n, ...) buffers: RAW (sanitised) states, standardised values / returns, normalised advantages.
        Returns (epoch KL means, learning rate)."""
        epochs = self.epochs if epochs is None else int(epochs)
        mbs = self.minibatches if minibatches is None else int(minibatches)
        obs = obs.reshape(-1, obs.shape[-1])
        B = obs.shape[0]
        act = act.reshape(B, -1)
        logp, val, ret, adv = (x.reshape(B) for x in (logp, val, ret, adv))
        params = list(self.policy.parameters()) + list(self.value.parameters())
        kls_out = []
        for epoch in range(epochs):
            perm = perms[epoch] if perms is not None else torch.randperm(B, device=self.device)
            kls = []
            for mb in perm.chunk(mbs):
                with torch.no_grad():
                    s = self.state_preprocessor(obs[mb], train=train_state_scaler and not epoch)
                loss, kl = ppo_loss(self.policy, self.value, s, act[mb], logp[mb], val[mb], ret[mb], adv[mb])
                kls.append(kl)
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                nn.utils.clip_grad_norm_(params, self.max_grad_norm)
                self.opt.step()
            kl_mean = torch.stack(kls).mean().item()
            kls_out.append(kl_mean)
            lr = kl_adaptive(self.lr, kl_mean)
            for g in self.opt.param_groups:
                g["lr"] = lr
        return kls_out, self.lr

    def state_dict(self) -> dict:
        return {"policy": self.policy.state_dict(), "value": self.value.state_dict(),
                STATE_KEY: self.state_preprocessor.state_dict(), VALUE_KEY: self.value_preprocessor.state_dict()}


# ---------------------------------------------------------------------------------------------------------------- HIP path
class FusedScaledPPO:
    """``FusedPPO`` behind a state scaler and a value scaler, everything on the device.  ``.actor`` / ``.critic`` / ``.log_std``
    are the inner trainer's and read STANDARDISED states (``state_scaler.forward``); the critic's output is on the standardised
    scale (``value_scaler.inverse`` gives values).  ``rollout_scaled.ScaledRolloutCollector`` does both per env step."""

    def __init__(self, policy_sd: Mapping[str, torch.Tensor], value_sd: Mapping[str, torch.Tensor], device="cuda", **kw):
        require_gpu("FusedScaledPPO", "TorchScaledPPO is the specification")
        self.inner = FusedPPO(policy_sd, value_sd, device=device, **kw)
        self.device = self.inner.device
        self.state_scaler = DeviceScaler(OBS_DIM, self.device)
        self.value_scaler = DeviceScaler(1, self.device)
        self._image = torch.empty(0, OBS_DIM, dtype=torch.float32, device=self.device)

    @classmethod
    def from_checkpoint(cls, ck, **kw) -> "FusedScaledPPO":
        """skrl checkpoint ``{"policy", "value"[, "state_preprocessor", "value_preprocessor"]}`` (a path or the loaded dict)."""
        ck = load_checkpoint(ck)
        t = cls(ck["policy"], ck["value"], **kw)
        for key, sc in ((STATE_KEY, t.state_scaler), (VALUE_KEY, t.value_scaler)):
            if key in ck:
                sc.load_state_dict(ck[key])
        return t

    # ---- the inner trainer's
    @property
    def actor(self):
        return self.inner.actor

    @property
    def critic(self):
        return self.inner.critic

    @property
    def log_std(self) -> torch.Tensor:
        return self.inner.log_std

    @property
    def params(self) -> torch.Tensor:
        return self.inner.params

    @property
    def lr(self) -> float:
        return self.inner.lr

    @property
    def steps(self) -> int:
        return self.inner.steps

    def gae(self, rew, done, val, last_v):
        """``FusedPPO.gae`` on values of the ORIGINAL scale (what the collector stores)."""
        return self.inner.gae(rew, done, val, last_v)

    def state_dict(self) -> dict:
        sd = self.inner.state_dict()
        sd[STATE_KEY], sd[VALUE_KEY] = self.state_scaler.state_dict(), self.value_scaler.state_dict()
        return sd

    # ---- the update
    def standardize_values(self, val: torch.Tensor, ret: torch.Tensor):
        """skrl PPO._update: the value scaler trains on the values and transforms them, then the same on the returns."""
        out = []
        for x in (val, ret):
            flat = x.reshape(-1, 1)
            self.value_scaler.train(flat)
            out.append(self.value_scaler.forward(flat).reshape(x.shape))
        return out[0], out[1]

    @property
    def last_update(self):
        return self.inner.last_update

    def update(self, obs, act, logp, val, ret, adv, perms=None, epochs: int | None = None, minibatches: int | None = None,
               train_state_scaler: bool = True, kl_early_stop: float = 0.0, scheduler: str | None = "kl_adaptive"):
        """``TorchScaledPPO.update`` on the device.  ``obs``: the RAW (sanitised) rows of the rollout buffer, never written;
        ``val`` / ``ret`` from ``standardize_values``.  Returns (epoch KLs, learning rate); one host synchronisation, at the end.
        ``kl_early_stop`` / ``scheduler`` as ``FusedPPO.update``: the gated path, the first epoch's scaler training included (the
        forward into the image runs ungated: rows written behind a stop are rewritten by the pass after the first epoch or never
        read)."""
        tr = self.inner
        gated = tr._gated(kl_early_stop, scheduler)
        epochs = tr.epochs if epochs is None else int(epochs)
        mbs = tr.minibatches if minibatches is None else int(minibatches)
        obs, act, logp, val, ret, adv, B = tr._flat_rollout(obs, act, logp=logp, val=val, ret=ret, adv=adv)
        if self._image.shape[0] < B:
            self._image = torch.empty(B, OBS_DIM, dtype=torch.float32, device=self.device)
        image = self._image[:B]
        gate = tr.epoch_state if gated else None

        def before(e, mb):
            if e == 0:                          # skrl: state_preprocessor(states, train=not epoch)
                if train_state_scaler:
                    self.state_scaler.train(obs, mb, gate=gate)
                self.state_scaler.forward(obs, mb, out=image)

        def after_first():                      # the statistics are final: one pass, then no scaler work in the later epochs
            if epochs > 1:
                self.state_scaler.forward(obs, out=image)

        return tr._epochs(image, act, logp, val, ret, adv, perms, epochs, mbs, gated, kl_early_stop, scheduler, before, after_first)
