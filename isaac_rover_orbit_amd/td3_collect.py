"""The off-policy half of an env step as library code: act, explore, store, sample (include/rover_td3_collect.h).

Per env step a TD3 trainer needs, around ``env.step`` (skrl's ``TD3.act`` + ``record_transition`` + ``RandomMemory.sample``; the loop
of ``examples/07_train_td3.py``): the actor's output on the current rows, optional Gaussian exploration noise and the clamp, the
transition (sanitised next rows, actions, reward, terminated) in the replay memory, and a batch of row indices.  ``TD3Collector``
does it in TWO HIP launches, writing straight into a ``td3.ReplayMemory``, in skrl's call order::

    col.begin(obs)                                    # rows after reset -> ring[cursor]
    loop:
        a = col.act(scale)                            # actor on ring[cursor], noise, clamp -> memory.actions[k] and the env's buffer
        obs, rew, term, trunc, info = env.step(a)
        idx = col.record(obs, rew, term, batch_size)  # sanitised rows -> ring[cursor + 1]; rew, term, ring_pos[k]; the indices
        fused.update(memory, idx)                     # the batch may hold the transition just added

The exploration noise and the batch indices are counter-based, like every draw of the env: Philox4x32-10 keyed by the
seed.  The noise is indexed by (global env id, counter, action pair) and the indices by (counter, position), so neither depends on
tensor shapes or on how the envs are split over ranks, and the checkpoint is ``{seed, counter, env_id_offset}``.  Every ``act`` and
every ``record`` takes the current counter for its draws and advances it by one, whether or not it draws.

``TorchTD3Collector`` is the same interface in plain torch / numpy: the specification of the kernels, and it runs on the CPU with
any callable as the actor.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _fused, _lib
from ._fused import f32_cuda, holds, launch, ptr
from .rollout import FLT_MAX, _MASK, philox4x32, standard_normals
from .td3 import OBS_DIM, ReplayMemory, explore

NOISE_TAG = 0x54443300            # "TD3\0": word 3 of the Philox counter of the exploration noise, | action pair
INDEX_TAG = 0x54335300            # "T3S\0": ... of the batch's row indices


# ---------------------------------------------------------------------------------------------------------------- the draws (spec)
def sample_indices(seed: int, counter: int, batch_size: int, mem_rows: int) -> np.ndarray:
    """int64 (batch_size,): position i takes word i & 3 of Philox4x32-10((i >> 2, counter_lo, counter_hi, INDEX_TAG), key = seed);
    the index is (word * mem_rows) >> 32, uniform over [0, mem_rows) up to 2**-32 mem_rows."""
    mem_rows = int(mem_rows)
    if not 1 <= mem_rows <= 2 ** 32:
        raise ValueError("mem_rows must lie in [1, 2**32]")
    i = np.arange(int(batch_size), dtype=np.uint64)
    w = philox4x32(i >> np.uint64(2), int(counter) & _MASK, (int(counter) >> 32) & _MASK, INDEX_TAG, int(seed) & _MASK,
                   (int(seed) >> 32) & _MASK)
    word = np.stack(w, axis=-1)[np.arange(i.size), (i & np.uint64(3)).astype(np.int64)]
    # word < 2**32 and mem_rows <= 2**32: the product is at most 2**64 - 2**32, which uint64 holds
    return ((word * np.uint64(mem_rows)) >> np.uint64(32)).astype(np.int64)


class _CollectorBase:
    """Counter, checkpoint, argument checks and the memory's bookkeeping shared by the two implementations."""

    def __init__(self, memory: ReplayMemory, seed: int, env_id_offset: int, noise_std: float, clip, state_scaler=None):
        if memory.obs.shape[-1] != OBS_DIM:
            raise ValueError(f"the memory must hold {OBS_DIM}-wide observations")
        self.memory = memory
        self.n, self.A = memory.num_envs, int(memory.actions.shape[-1])
        self.seed, self.env_id_offset, self.noise_std = int(seed), int(env_id_offset), float(noise_std)
        self.clip = (float(clip[0]), float(clip[1]))
        if self.noise_std < 0 or not self.clip[0] <= self.clip[1]:
            raise ValueError("noise_std must be >= 0 and clip = (low, high) with low <= high")
        self.counter = 0
        self.device = memory.device
        # skrl's state_preprocessor (offpolicy_scaled.py): the actor reads scaler(rows), untrained; the ring keeps the raw rows
        self.state_scaler = state_scaler

    def _states(self) -> torch.Tensor:
        """The rows the actor reads: the ring's cursor slot, through ``state_scaler`` (no training) when one was given."""
        rows = self.memory.obs[self.memory.cursor]
        return rows if self.state_scaler is None else self.state_scaler(rows)

    def state_dict(self) -> dict:
        """The checkpoint of the noise and of the batch indices: the counter, not a generator state."""
        return {"seed": self.seed, "counter": self.counter, "env_id_offset": self.env_id_offset}

    def load_state_dict(self, sd: dict) -> None:
        self.seed, self.counter, self.env_id_offset = int(sd["seed"]), int(sd["counter"]), int(sd["env_id_offset"])

    def _raw(self, raw_obs) -> torch.Tensor:
        if isinstance(raw_obs, dict):
            raw_obs = raw_obs["policy"]
        if raw_obs.dim() != 2 or tuple(raw_obs.shape) != (self.n, OBS_DIM) or raw_obs.dtype != torch.float32:
            raise ValueError(f"raw_obs must be a float32 tensor of shape ({self.n}, {OBS_DIM})")
        if raw_obs.device != self.memory.obs.device:
            raise ValueError(f"raw_obs must live on {self.memory.obs.device}")
        return raw_obs.contiguous()

    def _transition(self, rew, terminated):
        for name, x, dts in (("rew", rew, (torch.float32,)), ("terminated", terminated, (torch.bool, torch.uint8))):
            if x.dtype not in dts or not x.is_contiguous() or x.numel() != self.n or x.device != self.memory.obs.device:
                raise ValueError(f"{name} must be a contiguous {dts[0]} tensor of {self.n} elements on {self.memory.obs.device}")

    def _exploring(self, scale) -> bool:
        return scale is not None and self.noise_std != 0.0

    def _advance(self) -> None:
        """ReplayMemory.add's bookkeeping; a later plain ``add`` rewrites its states slot."""
        m = self.memory
        m.cursor = (m.cursor + 1) % m.slots
        m.memory_index += 1
        if m.memory_index >= m.memory_size:
            m.memory_index, m.filled = 0, True
        m._last_next, m._last_version = None, -1


# ------------------------------------------------------------------------------------------------------------------ the spec
class TorchTD3Collector(_CollectorBase):
    """The specification, in plain torch / numpy.  ``actor``: any callable (n, 965) -> (n, A)."""

    def __init__(self, actor, memory: ReplayMemory, seed: int = 42, env_id_offset: int = 0, noise_std: float = 0.0, clip=(-1.0, 1.0),
                 state_scaler=None):
        """``state_scaler``: a callable rows -> standardised rows (``lift_ppo.RunningStandardScaler``) or ``None``."""
        super().__init__(memory, seed, env_id_offset, noise_std, clip, state_scaler)
        self.actor = actor

    @staticmethod
    def sanitise(raw_obs: torch.Tensor) -> torch.Tensor:
        return torch.nan_to_num(raw_obs, nan=0.0, posinf=FLT_MAX, neginf=0.0)

    def draws(self, counter: int | None = None) -> np.ndarray:
        """float64 eps (n, A) of ``counter`` (default: the next call's)."""
        ids = self.env_id_offset + np.arange(self.n, dtype=np.int64)
        return standard_normals(self.seed, ids, self.counter if counter is None else counter, self.A, tag=NOISE_TAG)

    @torch.no_grad()
    def begin(self, raw_obs) -> None:
        m = self.memory
        m.obs[m.cursor] = self.sanitise(self._raw(raw_obs))
        m._last_next, m._last_version = None, -1

    @torch.no_grad()
    def act(self, scale: float | None = None) -> torch.Tensor:
        m = self.memory
        a = self.actor(self._states())
        if self._exploring(scale):
            eps = torch.from_numpy(self.draws().astype(np.float32)).to(a.device)
            a = explore(a, self.noise_std * eps, float(scale), *self.clip)
        m.actions[m.memory_index] = a
        self.counter += 1
        return a

    @torch.no_grad()
    def record(self, raw_obs, rew, terminated, batch_size: int | None = None):
        m = self.memory
        raw = self._raw(raw_obs)
        self._transition(rew, terminated)
        k, w = m.memory_index, m.cursor
        m.obs[(w + 1) % m.slots] = self.sanitise(raw)
        m.rewards[k] = rew.reshape(self.n)
        m.terminated[k] = terminated.reshape(self.n) != 0
        m.ring_pos[k] = w
        self._advance()
        idx = None
        if batch_size is not None:
            idx = torch.from_numpy(sample_indices(self.seed, self.counter, batch_size, len(m))).to(m.device)
        self.counter += 1
        return idx


# ---------------------------------------------------------------------------------------------------------------- the kernels
def default_hparams() -> "_lib.Td3CollectHparams":
    return _fused.default_hparams(_lib.Td3CollectHparams, "rover_td3_collect_default_hparams")


def _launch_act(fn: str, actor, rows: torch.Tensor, width: int, wide, narrow, *args) -> None:
    """The checks of an act wrapper, then ``launch(fn, rows.device, *args)``: ``rows`` (n, 965); ``wide`` pairs (name, tensor of
    (n, width) values); ``narrow`` triples (name, tensor, number of values).  Every tensor may be ``None``."""
    device = actor.packed.device
    f32_cuda("rows", rows, device)
    for name, t, _ in narrow:
        f32_cuda(name, t, device)
    for name, t in wide:
        f32_cuda(name, t, device)
    n = int(rows.shape[0])
    if rows.dim() != 2 or rows.shape[1] != OBS_DIM:
        raise ValueError(f"rows must have shape (n, {OBS_DIM})")
    for name, t in wide:
        holds(name, t, (n, width))
    for name, t, numel in narrow:
        holds(name, t, numel)
    launch(fn, rows.device, *args)


def collect_act(actor, rows: torch.Tensor, counter: int, hp: "_lib.Td3CollectHparams", act_out: torch.Tensor,
                env_act_out: torch.Tensor, *, mean_out=None, eps_out=None) -> None:
    """One ``rover_td3_collect_act`` launch on the current stream over the already-sanitised ``rows`` (n, 965); ``mean_out`` /
    ``eps_out`` left ``None`` are passed as NULL."""
    wide = (("act_out", act_out), ("env_act_out", env_act_out), ("mean_out", mean_out), ("eps_out", eps_out))
    _launch_act("rover_td3_collect_act", actor, rows, actor.out_dim, wide, (), C.byref(actor.desc), actor.packed.data_ptr(),
                actor.n_copies, C.byref(hp), C.c_uint64(int(counter)), rows.data_ptr(), int(rows.shape[0]), ptr(mean_out),
                act_out.data_ptr(), env_act_out.data_ptr(), ptr(eps_out))


def collect_record(raw: torch.Tensor, ring_slot: torch.Tensor, hp: "_lib.Td3CollectHparams", counter: int = 0, *, rew=None,
                   terminated=None, rew_out=None, term_out=None, ring_pos_entry=None, ring_pos_value: int = 0, idx_out=None,
                   mem_rows: int = 0) -> None:
    """One ``rover_td3_collect_record`` launch on the current stream; every argument left ``None`` is passed as NULL."""
    launch("rover_td3_collect_record", raw.device, raw.data_ptr(), int(raw.shape[0]), ring_slot.data_ptr(), ptr(rew), ptr(terminated),
           ptr(rew_out), ptr(term_out), ptr(ring_pos_entry), int(ring_pos_value), ptr(idx_out),
           0 if idx_out is None else int(idx_out.numel()), int(mem_rows), C.byref(hp), C.c_uint64(int(counter)))


class _FusedCollector(_CollectorBase):
    """What the fused collectors share: the env's action buffer, ``begin``, ``record`` and the seed / offset part of the hparams.
    A subclass names itself in ``_NAME``, launches its record kernel in ``_record`` and, with ``_DRAWS``, has ``record`` fill and
    return the update's (batch, 4) standard normals beside the indices."""

    _NAME = ""
    _DRAWS = False

    def __init__(self, memory: ReplayMemory, seed: int, env_id_offset: int, noise_std: float, clip, state_scaler=None):
        _fused.require_gpu(self._NAME, f"Torch{self._NAME} is the CPU specification")
        super().__init__(memory, seed, env_id_offset, noise_std, clip, state_scaler)
        self._scaled = None

    def _bind(self, actor) -> None:
        self._lib = _lib.load()
        self.actor = actor
        if self.memory.obs.device != actor.packed.device:
            raise ValueError("the memory must live on the actor's device")
        self._env_act = torch.zeros(self.n, self.A, dtype=torch.float32, device=self.memory.obs.device)
        self._bufs: dict = {}

    def _seeded(self, hp):
        return _fused.seeded(hp, self.seed, self.env_id_offset)

    def _states(self) -> torch.Tensor:
        """The rows the act kernel reads: the ring's cursor slot, or with a ``state_scaler`` (a ``scaler.DeviceScaler``) a scratch
        image that one ``rover_scaler_apply`` fills from it.  The slot itself is never written."""
        rows = self.memory.obs[self.memory.cursor]
        if self.state_scaler is None:
            return rows
        if self._scaled is None:
            self._scaled = torch.empty_like(rows)
        return self.state_scaler.forward(rows, out=self._scaled)

    def _record(self, raw, ring_slot, counter=0, idx=None, eps=None, **transition) -> None:
        raise NotImplementedError

    @torch.no_grad()
    def begin(self, raw_obs) -> None:
        """The rows after a reset go, sanitised, into the ring's cursor slot.  No draw: the counter stays."""
        m = self.memory
        self._record(self._raw(raw_obs), m.obs[m.cursor])
        m._last_next, m._last_version = None, -1

    @torch.no_grad()
    def record(self, raw_obs, rew: torch.Tensor, terminated: torch.Tensor, batch_size: int | None = None):
        """The transition of the step just taken: the env's rows, sanitised, into the next ring slot, reward / terminated / ring_pos of
        memory slot k; with ``batch_size`` the int64 row indices of a batch over the memory INCLUDING this transition -- with
        ``_DRAWS`` the pair ``(idx, eps)``, eps the update's float32 draws (batch_size, 4) -- else ``None``.  Advances the memory as
        ``ReplayMemory.add`` does, and the counter by one."""
        m = self.memory
        raw = self._raw(raw_obs)
        self._transition(rew, terminated)
        if not rew.is_cuda:
            raise ValueError("rew and terminated must be cuda tensors")
        if batch_size is not None and int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        k, w = m.memory_index, m.cursor
        self._advance()
        idx = eps = None
        if batch_size is not None:
            batch = int(batch_size)
            if batch not in self._bufs:
                self._bufs[batch] = (torch.zeros(batch, dtype=torch.int64, device=m.obs.device),
                                     torch.zeros(batch, 4, dtype=torch.float32, device=m.obs.device) if self._DRAWS else None)
            idx, eps = self._bufs[batch]
        self._record(raw, m.obs[(w + 1) % m.slots], self.counter, idx, eps, rew=rew, terminated=terminated, rew_out=m.rewards[k],
                     term_out=m.terminated[k], ring_pos_entry=m.ring_pos[k:k + 1], ring_pos_value=w, mem_rows=len(m))
        self.counter += 1
        return (idx, eps) if self._DRAWS and idx is not None else idx


class TD3Collector(_FusedCollector):
    """The fused collector: ``actor`` is a ``RoverNet`` (reference architecture, no final activation) and ``memory`` a
    ``ReplayMemory`` on the same device, both held BY REFERENCE -- with ``FusedTD3.actor`` the collector always sees the trainer's
    current parameters.  ``act`` returns a buffer the next call overwrites, ``record`` likewise (one index buffer per batch size).
    ``state_scaler``: a ``scaler.DeviceScaler`` (skrl's ``state_preprocessor``, ``offpolicy_scaled``): ``act`` then runs the actor on
    ``scaler.forward`` of the cursor slot, one more launch, and the ring keeps the raw rows; ``None``: the launches as they were.
    """

    _NAME = "TD3Collector"

    def __init__(self, actor, memory: ReplayMemory, seed: int = 42, env_id_offset: int = 0, noise_std: float = 0.0, clip=(-1.0, 1.0),
                 state_scaler=None):
        super().__init__(memory, seed, env_id_offset, noise_std, clip, state_scaler)
        self._bind(actor)
        if actor.out_dim != self.A or actor.out_dim > 16:
            raise ValueError("the memory's action width must be the actor's output width (at most 16)")

    def hparams(self, scale: float | None = None) -> "_lib.Td3CollectHparams":
        hp = self._seeded(default_hparams())
        hp.explore = int(self._exploring(scale))
        hp.noise_std, hp.noise_scale = self.noise_std, 1.0 if scale is None else float(scale)
        hp.action_low, hp.action_high = self.clip
        return hp

    def _record(self, raw, ring_slot, counter=0, idx=None, eps=None, **transition) -> None:
        collect_record(raw, ring_slot, self.hparams(), counter, idx_out=idx, **transition)

    @torch.no_grad()
    def act(self, scale: float | None = None, mean_out=None, eps_out=None) -> torch.Tensor:
        """The actor on the ring's cursor slot; ``scale`` is what ``td3.exploration_scale`` returns (``None``, or ``noise_std == 0``:
        the actor's output, not clamped).  Fills the memory's action slot and returns the actions for ``env.step``.  Advances the
        counter by one."""
        m = self.memory
        collect_act(self.actor, self._states(), self.counter, self.hparams(scale), m.actions[m.memory_index], self._env_act,
                    mean_out=mean_out, eps_out=eps_out)
        self.counter += 1
        return self._env_act
