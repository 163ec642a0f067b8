"""Fused PPO update of the rover's actor and critic on the MI355X (C ABI: ``include/rover_train.h``).

``FusedPPO`` holds both networks of the reference architecture (``policy.RoverNet``'s shapes) and ``log_std`` in ONE flat device
vector in the packed layout the forward kernels read, with Adam's moments beside it, and runs what ``examples/04_train_ppo.py``
does with torch autograd: GAE, then epochs of shuffled minibatches of the clipped PPO loss, ``clip_grad_norm_`` and Adam, with
the KL-adaptive learning rate after each epoch.  ``.actor`` / ``.critic`` alias the trainer's parameters (replicas refreshed by
every optimiser step), so a rollout needs no re-packing.  No CPU fallback.

``update(kl_early_stop=0.008, scheduler=None)`` is rover_ppo.yaml as skrl 1.1 reads it (``include/rover_train_gate.h``): an epoch
stops at the first minibatch whose KL exceeds the threshold, before that minibatch's optimiser step, and no scheduler touches the
learning rate.  The stop is one word of device memory that the kernels set and obey; the host still synchronises once.
``ppo_skrl.TorchSkrlPPO`` is the specification.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping

import torch

from . import _fused, _lib
from ._fused import ptr
from .policy import ENCODER_KEY, MLP_KEY, make_desc

LOG_STD_KEY = "log_std_parameter"


def default_hparams() -> "_lib.PpoHparams":
    return _fused.default_hparams(_lib.PpoHparams, "rover_ppo_default_hparams")


def _layers(sd: Mapping[str, torch.Tensor]):
    ws, bs, (n_enc, _) = _fused.host_layers(sd, (ENCODER_KEY, MLP_KEY))
    return ws, bs, n_enc


def pack(sd: Mapping[str, torch.Tensor], final_act: str):
    """(descriptor, packed host array) of a reference state_dict, exactly as ``RoverNet`` packs it."""
    ws, bs, n_enc = _layers(sd)
    desc = make_desc([w.shape for w in ws], n_enc, final_act, 965, 4, 0.01)
    return desc, _fused.pack_layers(desc, ws, bs)


def unpack(desc: "_lib.PolicyDesc", packed) -> dict:
    """Packed buffer (one replica) -> reference state_dict entries (``rover_policy_unpack``), float32 CPU tensors."""
    sd = {}
    for i, (w, b) in enumerate(zip(*_fused.unpack_layers(desc, packed))):
        key = ENCODER_KEY.format(2 * i, "{}") if i < desc.n_enc else MLP_KEY.format(2 * (i - desc.n_enc), "{}")
        sd[key.format("weight")], sd[key.format("bias")] = w, b
    return sd


class FusedPPO(_fused.FusedActorCritic):
    """PPO trainer state on the GPU: parameters, Adam moments, learning rate and step count all in device memory.

    ``lr`` and the hyper-parameters default to examples/04_train_ppo.py (rover_ppo.yaml).  ``update`` synchronises with the host
    once, at its end, to return the epoch KLs and the learning rate.  ``from_checkpoint`` takes a skrl checkpoint
    ``{"policy": state_dict, "value": state_dict, ...}`` (a path or the loaded dict).
    """

    _STATE, _WORKSPACE, _PARAM_FLOATS = _lib.PpoState, "rover_ppo_workspace_bytes", "rover_ppo_param_floats"
    _RUNS = "the reference architecture only (rover_train.h)"
    _PAD = 2
    _unpack = staticmethod(unpack)

    def __init__(self, policy_sd: Mapping[str, torch.Tensor], value_sd: Mapping[str, torch.Tensor], lr: float = 1e-4,
                 epochs: int = 4, minibatches: int = 60, device="cuda", n_copies: int = 4, **hparams):
        super().__init__(default_hparams, hparams, device, n_copies)
        self.epochs, self.minibatches = int(epochs), int(minibatches)
        self._networks(pack(policy_sd, "tanh"), pack(value_sd, "none"), policy_sd[LOG_STD_KEY])
        self.state = torch.zeros(4, dtype=torch.float64, device=self.device)   # struct rover_ppo_state (32 bytes)
        self.state[0] = float(lr)
        self.epoch_state = torch.zeros(8, dtype=torch.int32, device=self.device)    # struct rover_ppo_epoch (32 bytes), zeroed
        self.last_update = None                                                 # per-epoch {"recorded", "stopped"} of a gated update
        self._ensure_ws(1)

    # ---- views
    @property
    def lr(self) -> float:
        return float(self.state[0].item())

    @property
    def steps(self) -> int:
        return int(self.state.view(torch.int32)[2].item())

    # ---- kernels
    def minibatch(self, obs, act, logp, val, ret, adv, idx, stats=None, mean_out=None, value_out=None) -> torch.Tensor:
        """Gradient of one minibatch into ``self.grad``; ``stats`` (4 floats: KL, policy loss, value loss, 0)."""
        self._check(idx, "idx", torch.int64)
        n = int(idx.numel())
        self._ensure_ws(max(n, 1))
        if stats is None:
            stats = torch.empty(4, device=self.device)
        _lib.check(self._lib.rover_ppo_minibatch(C.byref(self.desc_p), C.byref(self.desc_v), C.byref(self.hp), self.params.data_ptr(),
                                                 obs.data_ptr(), act.data_ptr(), logp.data_ptr(), val.data_ptr(), ret.data_ptr(),
                                                 adv.data_ptr(), idx.data_ptr(), n, self.ws.data_ptr(), self.ws.numel(),
                                                 self.grad.data_ptr(), stats.data_ptr(), ptr(mean_out), ptr(value_out),
                                                 self._stream()), "rover_ppo_minibatch")
        return stats

    def apply(self):
        """clip_grad_norm_ + Adam on ``self.grad``, then the replicas ``.actor`` / ``.critic`` read."""
        _lib.check(self._lib.rover_ppo_apply(C.byref(self.desc_p), C.byref(self.desc_v), C.byref(self.hp), self.params.data_ptr(),
                                             self.grad.data_ptr(), self.adam_m.data_ptr(), self.adam_v.data_ptr(), self.state.data_ptr(),
                                             self.rep_p.data_ptr(), self.rep_v.data_ptr(), self.n_copies, self.ws.data_ptr(),
                                             self.ws.numel(), self._stream()), "rover_ppo_apply")

    def minibatch_gated(self, obs, act, logp, val, ret, adv, idx, stats, kl_early_stop: float = 0.0, mean_out=None, value_out=None):
        """``minibatch`` behind ``epoch_state``'s stop word (``rover_ppo_minibatch_gated``): nothing is written once it is set;
        otherwise the KL is recorded and sets the word where it exceeds ``kl_early_stop`` (> 0)."""
        self._check(idx, "idx", torch.int64)
        n = int(idx.numel())
        self._ensure_ws(max(n, 1))
        _lib.check(self._lib.rover_ppo_minibatch_gated(C.byref(self.desc_p), C.byref(self.desc_v), C.byref(self.hp),
                                                       self.params.data_ptr(), obs.data_ptr(), act.data_ptr(), logp.data_ptr(),
                                                       val.data_ptr(), ret.data_ptr(), adv.data_ptr(), idx.data_ptr(), n,
                                                       self.ws.data_ptr(), self.ws.numel(), self.grad.data_ptr(), stats.data_ptr(),
                                                       ptr(mean_out), ptr(value_out), float(kl_early_stop),
                                                       self.epoch_state.data_ptr(), self._stream()), "rover_ppo_minibatch_gated")
        return stats

    def apply_gated(self):
        """``apply`` behind the stop word: no step, nothing written, once it is set (``rover_ppo_apply_gated``)."""
        _lib.check(self._lib.rover_ppo_apply_gated(C.byref(self.desc_p), C.byref(self.desc_v), C.byref(self.hp), self.params.data_ptr(),
                                                   self.grad.data_ptr(), self.adam_m.data_ptr(), self.adam_v.data_ptr(),
                                                   self.state.data_ptr(), self.rep_p.data_ptr(), self.rep_v.data_ptr(), self.n_copies,
                                                   self.ws.data_ptr(), self.ws.numel(), self.epoch_state.data_ptr(), self._stream()),
                   "rover_ppo_apply_gated")

    def epoch_end(self, stats: torch.Tensor, schedule: bool, kl_out: torch.Tensor | None = None):
        """Closes a gated epoch on the device: the mean of the recorded KLs into ``kl_out``, the KL-adaptive rate when ``schedule``,
        and the stop word cleared (``rover_ppo_epoch_end``)."""
        self._check(stats, "stats")
        _lib.check(self._lib.rover_ppo_epoch_end(C.byref(self.hp), stats.data_ptr(), int(stats.shape[0]), self.state.data_ptr(),
                                                 self.epoch_state.data_ptr(), int(bool(schedule)),
                                                 None if kl_out is None else kl_out.data_ptr(), self._stream()), "rover_ppo_epoch_end")

    @staticmethod
    def _gated(kl_early_stop: float, scheduler) -> bool:
        """Whether ``update`` takes the gated entries; the defaults (0, "kl_adaptive") keep the ungated launch sequence."""
        if scheduler not in (None, "kl_adaptive"):
            raise ValueError('scheduler must be None or "kl_adaptive"')
        if not float(kl_early_stop) >= 0.0:
            raise ValueError("kl_early_stop must be >= 0 (0: no early stop)")
        return float(kl_early_stop) > 0.0 or scheduler is None

    def _finish_gated(self, kls: torch.Tensor, snaps: torch.Tensor):
        """The one synchronisation of a gated update: the epoch KLs, the per-epoch stop word / record count (snapshots of
        ``epoch_state`` taken on the stream before each ``epoch_end``) and the learning rate in one copy.  Returns (KLs, lr)."""
        E = kls.numel()
        host = torch.cat([kls.view(torch.int32), snaps[:, 0], snaps[:, 1], self.state[:1].view(torch.int32)]).cpu()
        self.last_update = {"recorded": host[2 * E:3 * E].tolist(), "stopped": [bool(x) for x in host[E:2 * E].tolist()]}
        return host[:E].view(torch.float32).tolist(), float(host[3 * E:].clone().view(torch.float64)[0])

    def kl_schedule(self, stats: torch.Tensor, kl_out: torch.Tensor | None = None):
        """KL-adaptive learning rate from the (n_minibatches, 4) stats of one epoch, on the device."""
        self._check(stats, "stats")
        _lib.check(self._lib.rover_ppo_kl_schedule(C.byref(self.hp), stats.data_ptr(), int(stats.shape[0]), self.state.data_ptr(),
                                                   None if kl_out is None else kl_out.data_ptr(), self._stream()),
                   "rover_ppo_kl_schedule")

    def update(self, obs, act, logp, val, ret, adv, perms=None, epochs: int | None = None, minibatches: int | None = None,
               kl_early_stop: float = 0.0, scheduler: str | None = "kl_adaptive"):
        """The example's PPO update on flat (B, ...) or (T, n_envs, ...) rollout buffers: ``epochs`` passes over
        ``torch.randperm(B).chunk(minibatches)`` (or the given ``perms[epoch]``).  Returns (epoch KLs, learning rate).

        ``kl_early_stop`` > 0: skrl's KL early stop (its ``kl_threshold``); ``scheduler=None``: no learning-rate scheduler.  Either
        takes the gated kernels: the launches are enqueued for every minibatch and those behind a stop return at once, the epoch
        KLs are the means over the recorded minibatches, and ``last_update`` holds per-epoch ``recorded`` / ``stopped``.  Still one
        host synchronisation, at the end.  ``last_stats`` keeps the (epochs, minibatches, 4) records on the device, NaN behind a
        stop."""
        gated = self._gated(kl_early_stop, scheduler)
        epochs = self.epochs if epochs is None else int(epochs)
        mbs = self.minibatches if minibatches is None else int(minibatches)
        obs, act, logp, val, ret, adv, _ = self._flat_rollout(obs, act, logp=logp, val=val, ret=ret, adv=adv)
        return self._epochs(obs, act, logp, val, ret, adv, perms, epochs, mbs, gated, kl_early_stop, scheduler)

    def _epochs(self, rows, act, logp, val, ret, adv, perms, epochs: int, mbs: int, gated: bool, kl_early_stop: float, scheduler,
                before=None, after_first=None):
        """The epoch loop of ``update`` on checked flat buffers; ``rows`` is what the networks read.  ``before(epoch, idx)`` runs
        ahead of each minibatch's launches and ``after_first()`` behind the first epoch's minibatches (``FusedScaledPPO``'s scaler
        work)."""
        B = rows.shape[0]
        kls = torch.empty(epochs, device=self.device)
        if gated:                                   # records behind a stop are never written: they stay NaN
            stats = torch.full((epochs, mbs, 4), float("nan"), device=self.device)
            self.epoch_state.zero_()
            snaps = torch.empty(epochs, 8, dtype=torch.int32, device=self.device)
        else:
            stats = torch.empty(epochs, mbs, 4, device=self.device)
        self.last_stats = stats                     # (epochs, minibatches, 4): KL, policy loss, value loss, 0 per minibatch
        for e in range(epochs):
            for j, mb in enumerate(self._minibatches(perms, e, B, mbs)):
                mb = mb.contiguous()
                if before is not None:
                    before(e, mb)
                if gated:
                    self.minibatch_gated(rows, act, logp, val, ret, adv, mb, stats[e, j], kl_early_stop)
                    self.apply_gated()
                else:
                    self.minibatch(rows, act, logp, val, ret, adv, mb, stats=stats[e, j])
                    self.apply()
            if e == 0 and after_first is not None:
                after_first()
            if gated:
                snaps[e].copy_(self.epoch_state)
                self.epoch_end(stats[e], scheduler is not None, kls[e:e + 1])
            else:
                self.kl_schedule(stats[e], kls[e:e + 1])
        if gated:
            return self._finish_gated(kls, snaps)
        self.last_update = None
        return kls.cpu().tolist(), self.lr
