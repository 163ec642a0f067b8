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

import numpy as np
import torch

from . import _lib
from .policy import ENCODER_KEY, MLP_KEY, RoverNet, make_desc

LOG_STD_KEY = "log_std_parameter"


def default_hparams() -> "_lib.PpoHparams":
    h = _lib.PpoHparams()
    _lib.check(_lib.load().rover_ppo_default_hparams(C.byref(h)), "rover_ppo_default_hparams")
    return h


def _layers(sd: Mapping[str, torch.Tensor]):
    ws, bs, n_enc = [], [], 0
    while ENCODER_KEY.format(2 * n_enc, "weight") in sd:
        ws.append(sd[ENCODER_KEY.format(2 * n_enc, "weight")]); bs.append(sd[ENCODER_KEY.format(2 * n_enc, "bias")])
        n_enc += 1
    i = 0
    while MLP_KEY.format(2 * i, "weight") in sd:
        ws.append(sd[MLP_KEY.format(2 * i, "weight")]); bs.append(sd[MLP_KEY.format(2 * i, "bias")])
        i += 1
    ws = [np.ascontiguousarray(torch.as_tensor(w).detach().cpu().numpy(), dtype=np.float32) for w in ws]
    bs = [np.ascontiguousarray(torch.as_tensor(b).detach().cpu().numpy(), dtype=np.float32) for b in bs]
    return ws, bs, n_enc


def pack(sd: Mapping[str, torch.Tensor], final_act: str):
    """(descriptor, packed host array) of a reference state_dict, exactly as ``RoverNet`` packs it."""
    ws, bs, n_enc = _layers(sd)
    desc = make_desc([w.shape for w in ws], n_enc, final_act, 965, 4, 0.01)
    lib = _lib.load()
    packed = np.empty(int(lib.rover_policy_packed_floats(C.byref(desc))), dtype=np.float32)
    nl = len(ws)
    wp = (C.c_void_p * nl)(*[w.ctypes.data for w in ws])
    bp = (C.c_void_p * nl)(*[b.ctypes.data for b in bs])
    _lib.check(lib.rover_policy_pack(C.byref(desc), wp, bp, packed.ctypes.data), "rover_policy_pack")
    return desc, packed


def unpack(desc: "_lib.PolicyDesc", packed) -> dict:
    """Packed buffer (one replica) -> reference state_dict entries (``rover_policy_unpack``), float32 CPU tensors."""
    packed = np.ascontiguousarray(torch.as_tensor(packed).detach().cpu().numpy(), dtype=np.float32)
    nl = desc.n_enc + desc.n_mlp
    ws = [np.empty((desc.layers[i].N, desc.layers[i].K), np.float32) for i in range(nl)]
    bs = [np.empty(desc.layers[i].N, np.float32) for i in range(nl)]
    wp = (C.c_void_p * nl)(*[w.ctypes.data for w in ws])
    bp = (C.c_void_p * nl)(*[b.ctypes.data for b in bs])
    _lib.check(_lib.load().rover_policy_unpack(C.byref(desc), packed.ctypes.data, wp, bp), "rover_policy_unpack")
    sd = {}
    for i in range(nl):
        key = ENCODER_KEY.format(2 * i, "{}") if i < desc.n_enc else MLP_KEY.format(2 * (i - desc.n_enc), "{}")
        sd[key.format("weight")] = torch.from_numpy(ws[i])
        sd[key.format("bias")] = torch.from_numpy(bs[i])
    return sd


class FusedPPO:
    """PPO trainer state on the GPU: parameters, Adam moments, learning rate and step count all in device memory.

    ``lr`` and the hyper-parameters default to examples/04_train_ppo.py (rover_ppo.yaml).  ``update`` synchronises with the host
    once, at its end, to return the epoch KLs and the learning rate.
    """

    def __init__(self, policy_sd: Mapping[str, torch.Tensor], value_sd: Mapping[str, torch.Tensor], lr: float = 1e-4,
                 epochs: int = 4, minibatches: int = 60, device="cuda", n_copies: int = 4, **hparams):
        if not torch.cuda.is_available():
            raise _lib.RoverHipError("FusedPPO needs a ROCm GPU (no CPU fallback)")
        self._lib = _lib.load()
        self.device = torch.device(device)
        self.hp = default_hparams()
        for k, v in hparams.items():
            if not hasattr(self.hp, k):
                raise TypeError(f"unknown hyper-parameter {k!r}")
            setattr(self.hp, k, v)
        self.epochs, self.minibatches, self.n_copies = int(epochs), int(minibatches), int(n_copies)
        self.desc_p, pa = pack(policy_sd, "tanh")
        self.desc_v, pv = pack(value_sd, "none")
        P = int(self._lib.rover_ppo_param_floats(C.byref(self.desc_p), C.byref(self.desc_v)))
        if P == 0:
            raise _lib.RoverHipError("FusedPPO runs the reference architecture only (rover_train.h)")
        self.n_p, self.n_v = pa.size, pv.size
        ls = torch.as_tensor(policy_sd[LOG_STD_KEY]).detach().float().cpu().reshape(-1)
        if ls.numel() != 2:
            raise ValueError("log_std_parameter must hold 2 values")
        flat = np.concatenate([pa, pv, ls.numpy(), np.zeros(2, np.float32)])
        assert flat.size == P
        self.params = torch.from_numpy(flat).to(self.device)
        self.grad = torch.zeros_like(self.params)
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        self.state = torch.zeros(4, dtype=torch.float64, device=self.device)   # struct rover_ppo_state (32 bytes)
        self.state[0] = float(lr)
        self.epoch_state = torch.zeros(8, dtype=torch.int32, device=self.device)    # struct rover_ppo_epoch (32 bytes), zeroed
        self.last_update = None                                                 # per-epoch {"recorded", "stopped"} of a gated update
        self.rep_p = self.params[:self.n_p].repeat(self.n_copies)
        self.rep_v = self.params[self.n_p:self.n_p + self.n_v].repeat(self.n_copies)
        self.actor = RoverNet.from_packed(self.desc_p, self.rep_p, self.n_copies)
        self.critic = RoverNet.from_packed(self.desc_v, self.rep_v, self.n_copies)
        self.ws = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._ensure_ws(1)

    @classmethod
    def from_checkpoint(cls, ck, **kw) -> "FusedPPO":
        """skrl checkpoint ``{"policy": state_dict, "value": state_dict, ...}`` (a path or the loaded dict)."""
        if isinstance(ck, str):
            ck = torch.load(ck, map_location="cpu", weights_only=False)
        return cls(ck["policy"], ck["value"], **kw)

    # ---- views
    @property
    def log_std(self) -> torch.Tensor:
        """The raw (unclamped) log_std parameter, a view of the device vector."""
        return self.params[self.n_p + self.n_v:self.n_p + self.n_v + 2]

    @property
    def lr(self) -> float:
        return float(self.state[0].item())

    @property
    def steps(self) -> int:
        return int(self.state.view(torch.int32)[2].item())

    def state_dict(self) -> dict:
        """``{"policy": ..., "value": ...}`` in the skrl / example layout (float32 CPU tensors)."""
        p = self.params.cpu()
        pol = unpack(self.desc_p, p[:self.n_p])
        pol[LOG_STD_KEY] = p[self.n_p + self.n_v:self.n_p + self.n_v + 2].clone()
        return {"policy": pol, "value": unpack(self.desc_v, p[self.n_p:self.n_p + self.n_v])}

    # ---- kernels
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _ensure_ws(self, rows: int):
        need = int(self._lib.rover_ppo_workspace_bytes(int(rows)))
        if self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)

    @staticmethod
    def _check(t: torch.Tensor, name: str, dtype=torch.float32):
        if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} cuda tensor")

    def gae(self, rew: torch.Tensor, done: torch.Tensor, val: torch.Tensor, last_v: torch.Tensor):
        """(adv, ret) of (T, n_envs) rollouts, bit-identical to the example's torch loop; adv is not normalised."""
        for t, nm in ((rew, "rew"), (done, "done"), (val, "val"), (last_v, "last_v")):
            self._check(t, nm)
        T, n = rew.shape
        adv, ret = torch.empty_like(rew), torch.empty_like(rew)
        _lib.check(self._lib.rover_ppo_gae(C.byref(self.hp), rew.data_ptr(), done.data_ptr(), val.data_ptr(), last_v.data_ptr(), T, n,
                                           adv.data_ptr(), ret.data_ptr(), self._stream()), "rover_ppo_gae")
        return adv, ret

    def minibatch(self, obs, act, logp, val, ret, adv, idx, stats=None, mean_out=None, value_out=None) -> torch.Tensor:
        """Gradient of one minibatch into ``self.grad``; ``stats`` (4 floats: KL, policy loss, value loss, 0)."""
        self._check(idx, "idx", torch.int64)
        n = int(idx.numel())
        self._ensure_ws(max(n, 1))
        if stats is None:
            stats = torch.empty(4, device=self.device)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
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
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
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
        obs = obs.reshape(-1, obs.shape[-1])
        B = obs.shape[0]
        act = act.reshape(B, -1)
        logp, val, ret, adv = (x.reshape(B) for x in (logp, val, ret, adv))
        for t, nm in ((obs, "obs"), (act, "act"), (logp, "logp"), (val, "val"), (ret, "ret"), (adv, "adv")):
            self._check(t, nm)
        if obs.shape[1] != 965 or act.shape[1] != 2:
            raise ValueError("obs must be (B, 965) and act (B, 2)")
        kls = torch.empty(epochs, device=self.device)
        if gated:                                   # records behind a stop are never written: they stay NaN
            stats = torch.full((epochs, mbs, 4), float("nan"), device=self.device)
            self.epoch_state.zero_()
            snaps = torch.empty(epochs, 8, dtype=torch.int32, device=self.device)
        else:
            stats = torch.empty(epochs, mbs, 4, device=self.device)
        self.last_stats = stats                     # (epochs, minibatches, 4): KL, policy loss, value loss, 0 per minibatch
        for e in range(epochs):
            perm = perms[e] if perms is not None else torch.randperm(B, device=self.device)
            chunks = perm.chunk(mbs)
            if len(chunks) != mbs:
                raise ValueError(f"{B} rows do not make {mbs} minibatches")
            for j, mb in enumerate(chunks):
                if gated:
                    self.minibatch_gated(obs, act, logp, val, ret, adv, mb.contiguous(), stats[e, j], kl_early_stop)
                    self.apply_gated()
                else:
                    self.minibatch(obs, act, logp, val, ret, adv, mb.contiguous(), stats=stats[e, j])
                    self.apply()
            if gated:
                snaps[e].copy_(self.epoch_state)
                self.epoch_end(stats[e], scheduler is not None, kls[e:e + 1])
            else:
                self.kl_schedule(stats[e], kls[e:e + 1])
        if gated:
            return self._finish_gated(kls, snaps)
        self.last_update = None
        return kls.cpu().tolist(), self.lr
