"""TD3 and SAC with skrl's running state scaler (``state_preprocessor`` of rover_td3.yaml / rover_sac.yaml; C ABI of the new
device path: ``include/rover_offpolicy_scaled.h``).

skrl 1.1 semantics, STATED FROM MEMORY as everything in ``td3.py`` (so the uncertain part is a hyper-parameter):

* ``act``: the policy sees ``state_preprocessor(states)`` without training; the memory keeps the raw (sanitised) states.  That is
  the collectors' ``state_scaler`` argument (``td3_collect``, ``td3_explore``, ``sac_collect``).
* ``_update``, after the batch is sampled: ``s = pre(s, train=True)`` then ``s' = pre(s', train=True)``, so ``s`` is standardised
  with the statistics after the first training and ``s'`` with those after both.  Everything behind that (target actor, critics,
  ``y``, actor step, SAC's head, alpha) runs on the standardised rows; rewards, actions and ``terminated`` are untouched.
* ``train_next_states`` (default True): later skrl versions train on ``s`` only; False standardises ``s'`` without a second training.
* ``gradient_steps`` stays 1.

``FusedScaledTD3`` / ``FusedScaledSAC`` compose an UNCHANGED ``td3.FusedTD3`` / ``sac.FusedSAC`` with a ``scaler.DeviceScaler``, the
way ``ppo_scaled.FusedScaledPPO`` composes ``FusedPPO``: one kernel resolves the sampled indices to ring rows and compacts the
transitions, the scaler trains on the ring rows where they lie, one kernel per side writes the standardised rows into a
``StagedBatch`` (a one-slot ``td3.ReplayMemory``), and the inner trainer updates on that with the identity index.  No host
synchronisation.  ``TorchScaledTD3`` / ``TorchScaledSAC`` are the specifications: ``TorchTD3`` / ``TorchSAC`` around
``lift_ppo.RunningStandardScaler`` in the same order, in float32 or float64.

The checkpoint carries skrl's ``state_preprocessor`` entry (``running_mean``, ``running_variance``, ``current_count``) beside the
trainer's keys; a checkpoint without it starts the block at mean 0, variance 1, count 1.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _fused
from ._fused import launch, load_checkpoint, require_gpu
from .lift_ppo import RunningStandardScaler
from .sac import FusedSAC, TorchSAC
from .scaler import DeviceScaler
from .td3 import OBS_DIM, FusedTD3, ReplayMemory, TorchTD3

STATE_KEY = "state_preprocessor"


# ---------------------------------------------------------------------------------------------------------------- torch spec
class _TorchScaled:
    """What the two specifications share: the scaler, ``policy`` and the standardised sample."""

    def __init__(self, inner, state_scaler=None, train_next_states: bool = True):
        self.inner = inner
        dev = next(inner.policy.parameters()).device
        self.state_preprocessor = RunningStandardScaler(OBS_DIM, device=dev) if state_scaler is None else state_scaler
        self.train_next_states = bool(train_next_states)

    @property
    def dtype(self):
        return self.inner.dtype

    def policy(self, states: torch.Tensor) -> torch.Tensor:
        """skrl ``act``: the policy on ``state_preprocessor(states)``, no training (SAC: the tanh mean)."""
        with torch.no_grad():
            return self.inner.policy(self.state_preprocessor(states.to(self.dtype)))

    def sample(self, memory: ReplayMemory, idx: torch.Tensor, train: bool = True):
        """(s, a, r, s', terminated) of the rows ``idx`` with ``s`` and ``s'`` standardised in skrl's order."""
        dt = self.dtype
        s, a, r, s2, t = memory.gather(idx)
        if train and s.shape[0] < 2:
            raise ValueError("training the state scaler needs at least two rows (the unbiased variance of one row is NaN)")
        with torch.no_grad():
            s = self.state_preprocessor(s.to(dt), train=train)
            s2 = self.state_preprocessor(s2.to(dt), train=train and self.train_next_states)
        return s, a.to(dt), r.to(dt), s2, t

    def checkpoint(self) -> dict:
        return {**self.inner.checkpoint(), STATE_KEY: self.state_preprocessor.state_dict()}

    def load_state_preprocessor(self, ck) -> None:
        """The ``state_preprocessor`` entry of a checkpoint; without one the statistics restart at mean 0, variance 1, count 1."""
        sc = self.state_preprocessor
        if STATE_KEY in ck:
            sc.load_state_dict(ck[STATE_KEY])
        else:
            fresh = RunningStandardScaler(sc.running_mean.numel(), device=sc.running_mean.device)
            sc.load_state_dict(fresh.state_dict())


class TorchScaledTD3(_TorchScaled):
    """``TorchTD3.update`` behind the state scaler (skrl TD3._update with a ``state_preprocessor``, stated from memory)."""

    def __init__(self, inner: TorchTD3, state_scaler=None, train_next_states: bool = True):
        super().__init__(inner, state_scaler, train_next_states)

    def update(self, memory: ReplayMemory, idx: torch.Tensor, noise: torch.Tensor | None = None, train: bool = True) -> dict:
        tr = self.inner
        s, a, r, s2, t = self.sample(memory, idx, train)
        st = tr.critic_step(s, a, r, s2, t, noise)
        st.pop("y")
        tr.critic_update_counter += 1
        st["actor_stepped"] = not tr.critic_update_counter % tr.hp["policy_delay"]
        if st["actor_stepped"]:
            st.update(tr.actor_step(s))
            tr.polyak()
        return st


class TorchScaledSAC(_TorchScaled):
    """``TorchSAC.update`` behind the state scaler (skrl SAC._update with a ``state_preprocessor``, stated from memory)."""

    def __init__(self, inner: TorchSAC, state_scaler=None, train_next_states: bool = True):
        super().__init__(inner, state_scaler, train_next_states)

    def update(self, memory: ReplayMemory, idx: torch.Tensor, eps: torch.Tensor, train: bool = True) -> dict:
        tr = self.inner
        s, a, r, s2, t = self.sample(memory, idx, train)
        st = tr.critic_step(s, a, r, s2, t, eps[:, 0:2])
        st.pop("y")
        st.update(tr.policy_step(s, eps[:, 2:4]))
        tr.polyak()
        return st


# ---------------------------------------------------------------------------------------------------------------- HIP path
class StagedBatch(ReplayMemory):
    """A ``ReplayMemory(memory_size=1, num_envs=n)`` that the staging kernels fill: ``obs[0]`` the standardised ``s``, ``obs[1]`` the
    standardised ``s'``, ``ring_pos[0] = 0``, filled (``len == n``).  With ``arange`` as the index the trainers' gather reads row i of
    the sample for batch position i.  ``rows_s`` / ``rows_next`` are the sample's ring rows in the memory it was drawn from."""

    def __init__(self, n: int, device="cuda"):
        super().__init__(1, int(n), device)
        self.filled = True
        self.arange = torch.arange(self.num_envs, dtype=torch.int64, device=self.device)
        self.rows_s = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)
        self.rows_next = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)


def stage_resolve(memory: ReplayMemory, idx: torch.Tensor, staged: StagedBatch, bad_index: torch.Tensor) -> None:
    """One ``rover_offpolicy_stage_resolve`` launch on the current stream: the ring rows of ``idx`` into ``staged.rows_s`` /
    ``rows_next`` and the compact transitions into its action / reward / terminated slot."""
    n = int(idx.numel())
    if n != staged.num_envs or staged.actions.shape[-1] != memory.actions.shape[-1]:
        raise ValueError("the staged batch does not have the sample's rows or the memory's action width")
    if not idx.is_cuda or idx.dtype != torch.int64 or not idx.is_contiguous() or idx.device != memory.obs.device:
        raise ValueError("idx must be a contiguous int64 cuda tensor on the memory's device")
    if bad_index.dtype != torch.int32 or bad_index.device != memory.obs.device or staged.obs.device != memory.obs.device:
        raise ValueError("bad_index must be an int32 tensor, and the staged batch must live, on the memory's device")
    launch("rover_offpolicy_stage_resolve", memory.obs.device, idx.data_ptr(), n, len(memory), memory.num_envs, memory.slots,
           memory.ring_pos.data_ptr(), memory.actions.data_ptr(), int(memory.actions.shape[-1]), memory.rewards.data_ptr(),
           memory.terminated.data_ptr(), staged.rows_s.data_ptr(), staged.rows_next.data_ptr(), staged.actions.data_ptr(),
           staged.rewards.data_ptr(), staged.terminated.data_ptr(), bad_index.data_ptr())


def stage_rows(scaler: DeviceScaler, x: torch.Tensor, src: torch.Tensor, out: torch.Tensor, bad_index: torch.Tensor | None = None) -> None:
    """One ``rover_offpolicy_stage_rows`` launch on the current stream: ``out[i] = scaler.forward(x.reshape(-1, width)[src[i]])`` for
    every entry of ``src``; ``out`` holds at least ``len(src)`` rows and does not overlap ``x``."""
    w, dev = scaler.width, scaler.block.device
    for name, t in (("x", x), ("out", out)):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.numel() % w:
            raise ValueError(f"{name} must be contiguous float32 rows of {w} columns on the scaler's device")
    if not src.is_cuda or src.dtype != torch.int64 or not src.is_contiguous() or src.device != dev or src.numel() < 1:
        raise ValueError("src must be a contiguous int64 cuda tensor on the scaler's device")
    n = int(src.numel())
    if out.numel() < n * w:
        raise ValueError(f"out must hold {n} rows")
    if bad_index is not None and (bad_index.dtype != torch.int32 or bad_index.device != dev):
        raise ValueError("bad_index must be an int32 tensor on the scaler's device")
    launch("rover_offpolicy_stage_rows", dev, C.byref(scaler.hp), scaler.block.data_ptr(), w, x.data_ptr(), x.numel() // w,
           src.data_ptr(), n, out.data_ptr(), _fused.ptr(bad_index))


class _FusedScaled:
    """What the two fused classes share.  ``fused`` is held by reference and used as it is; attributes not named here (``params``,
    ``target``, ``critic_updates``, ``log_std`` ...) are the inner trainer's."""

    _INNER = None

    def __init__(self, fused, state_scaler: DeviceScaler | None = None, train_next_states: bool = True):
        require_gpu(type(self).__name__, f"Torch{type(self).__name__[5:]} is the specification")
        if not isinstance(fused, self._INNER):
            raise TypeError(f"fused must be a {self._INNER.__name__}")
        self.fused = fused
        self.device = fused.params.device
        self.state_scaler = DeviceScaler(OBS_DIM, self.device) if state_scaler is None else state_scaler
        if self.state_scaler.width != OBS_DIM or self.state_scaler.block.device != self.device:
            raise ValueError(f"state_scaler must be a {OBS_DIM}-wide DeviceScaler on the trainer's device")
        self.train_next_states = bool(train_next_states)
        self.bad_index = torch.zeros(1, dtype=torch.int32, device=self.device)    # sticky, as the trainers' own
        self.staged: StagedBatch | None = None

    def __getattr__(self, name):
        if name == "fused":                     # not yet set: no recursion
            raise AttributeError(name)
        return getattr(self.fused, name)

    @classmethod
    def from_checkpoint(cls, ck, train_next_states: bool = True, **kw):
        """The inner trainer's checkpoint (a path or the loaded dict) with or without skrl's ``state_preprocessor`` entry."""
        ck = load_checkpoint(ck)
        t = cls(cls._INNER.from_checkpoint(ck, **kw), train_next_states=train_next_states)
        t.load_state_preprocessor(ck)
        return t

    def load_state_preprocessor(self, ck) -> None:
        """The ``state_preprocessor`` entry of a checkpoint; without one the block restarts at mean 0, variance 1, count 1."""
        sc = self.state_scaler
        if STATE_KEY in ck:
            sc.load_state_dict(ck[STATE_KEY])
        else:
            sc.block.zero_()
            sc.block[sc.width:] = 1.0

    @property
    def actor(self):
        """The inner trainer's actor; it reads STANDARDISED rows (the collectors' ``state_scaler`` argument)."""
        return self.fused.actor

    def state_dict(self) -> dict:
        sd = self.fused.state_dict()
        sd[STATE_KEY] = self.state_scaler.state_dict()
        return sd

    def stats(self) -> dict:
        """The inner trainer's state (one host synchronisation); ``bad_index`` also reports the staging's."""
        st = self.fused.stats()
        st["bad_index"] = int(st["bad_index"]) | int(self.bad_index.item() != 0)
        return st

    def stage(self, memory: ReplayMemory, idx: torch.Tensor, train: bool = True) -> StagedBatch:
        """Steps 1 to 5 of the header: resolve, train on ``s``, stage ``s``, train on ``s'`` (the switch), stage ``s'``."""
        n = _fused.FusedOffPolicy._sample(self.fused, memory, idx)
        if train and n < 2:
            raise ValueError("training the state scaler needs at least two rows (update(..., train=False) accepts one)")
        if self.staged is None or self.staged.num_envs != n:
            self.staged = StagedBatch(n, self.device)
        st, sc = self.staged, self.state_scaler
        stage_resolve(memory, idx, st, self.bad_index)
        if train:
            sc.train(memory.obs, st.rows_s)
        stage_rows(sc, memory.obs, st.rows_s, st.obs[0])
        if train and self.train_next_states:
            sc.train(memory.obs, st.rows_next)
        stage_rows(sc, memory.obs, st.rows_next, st.obs[1])
        return st


class FusedScaledTD3(_FusedScaled):
    """``FusedTD3`` behind the state scaler, everything on the device."""

    _INNER = FusedTD3

    def update(self, memory: ReplayMemory, idx: torch.Tensor, noise: torch.Tensor | None = None, train: bool = True) -> bool:
        """``TorchScaledTD3.update`` on the device (no host synchronisation); returns whether the actor stepped.  ``train=False``
        freezes the statistics."""
        st = self.stage(memory, idx, train)
        return self.fused.update(st, st.arange, noise)


class FusedScaledSAC(_FusedScaled):
    """``FusedSAC`` behind the state scaler, everything on the device."""

    _INNER = FusedSAC

    def update(self, memory: ReplayMemory, idx: torch.Tensor, eps: torch.Tensor, train: bool = True) -> None:
        """``TorchScaledSAC.update`` on the device (no host synchronisation).  ``train=False`` freezes the statistics."""
        st = self.stage(memory, idx, train)
        self.fused.update(st, st.arange, eps)
