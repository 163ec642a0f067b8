"""The off-policy half of a SAC env step as library code: act, sample, store, draw (include/rover_sac_collect.h).

Per env step a SAC trainer needs, around ``env.step`` (skrl's ``SAC.act`` on the Gaussian policy + ``record_transition`` +
``RandomMemory.sample``; the torch loop of ``examples/09_train_sac.py``): the tanh mean on the current rows, an action sampled from
the policy's own Gaussian head and clamped, the transition (sanitised next rows, actions, reward, terminated) in the replay memory,
a batch of row indices and the update's standard normal draws.  ``SACCollector`` does it in TWO HIP launches, writing straight into
a ``td3.ReplayMemory``, in ``TD3Collector``'s call order::

    col.begin(obs)                                      # rows after reset -> ring[cursor]
    loop:
        a = col.act(timestep)                           # actor on ring[cursor], draw, clamp -> memory.actions[k] and the env's buffer
        obs, rew, term, trunc, info = env.step(a)
        idx, eps = col.record(obs, rew, term, batch)    # sanitised rows -> ring[cursor + 1]; rew, term, ring_pos[k]; indices, draws
        fused.update(memory, idx, eps)                  # the batch may hold the transition just added

Every draw is counter-based, Philox4x32-10 keyed by the seed, with a word-3 tag of its own (``TAGS``; the header carries the full
table).  The action draws are indexed by (global env id, counter, action column), the indices and the update's draws by (counter,
batch position), so none depends on tensor shapes or on how the envs are split over ranks, and the checkpoint is
``{seed, counter, env_id_offset}``.  Every ``act`` and every ``record`` takes the current counter for its draws and advances it by
one, whether or not it draws.  The indices are ``td3_collect.sample_indices`` and the update's draws ``td3_explore.smooth_normals``
of width 4, as they stand: the kernel's outputs are bit-comparable with ``rover_td3_collect_record`` and ``rover_td3_smooth_draw``.

``TorchSACCollector`` is the same interface in torch / numpy: the specification of the kernels (``cephes_expf``, ``head`` and
``random_actions`` below are float32 numpy with the operation order written out), and it runs on the CPU with any callable as the
actor.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _fused, _lib
from ._fused import f32_cuda, launch, ptr
from .rollout import _MASK, philox4x32, standard_normals, unit_uniform
from .td3 import ACT_DIM, ReplayMemory
from .td3_collect import TorchTD3Collector, _FusedCollector, _launch_act
from .td3_explore import SAC_ACTION_TAG as ACTION_TAG  # "SAC\0": word 3 of the Philox counter of the action draws, | action pair
from .td3_explore import SAC_RANDOM_TAG as RANDOM_TAG  # "SAR\0": ... of the random steps' uniforms, | action quad
from .td3_explore import smooth_normals

TAGS = {"sac_action": ACTION_TAG, "sac_random": RANDOM_TAG}   # the two new streams; td3_explore.TAGS is the repository's table
SAMPLE, MEAN, RANDOM = _lib.SAC_COLLECT_SAMPLE, _lib.SAC_COLLECT_MEAN, _lib.SAC_COLLECT_RANDOM
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
HALF_LN_2PI = np.float32(0.91893853320467274178)
_F = np.float32


# ---------------------------------------------------------------------------------------------------------------- the head (spec)
def cephes_expf(x) -> np.ndarray:
    """``rv_expf`` of the kernels (Cephes expf) restated in float32 numpy, every product and sum rounded to float32 in the kernels'
    order.  A NaN stays a NaN; above 88 the result is inf, below -88 it is 0."""
    x = np.asarray(x, dtype=_F)
    nan, big, small = np.isnan(x), x > _F(88.0), x < _F(-88.0)
    v = np.where(nan | big | small, _F(0.0), x).astype(_F)
    z = np.floor(_F(1.44269504088896341) * v + _F(0.5))
    v = v - z * _F(0.693359375)
    v = v - z * _F(-2.12194440e-4)
    zz = v * v
    p = _F(1.9875691500e-4)
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = p * v + _F(c)
    p = (p * zz + v) + _F(1.0)
    out = np.ldexp(p.astype(_F), z.astype(np.int32)).astype(_F)
    out = np.where(big, _F(np.inf), np.where(small, _F(0.0), out))
    return np.where(nan, _F(np.nan), out).astype(_F)


def tclamp(x, lo: float, hi: float) -> np.ndarray:
    """torch.clamp in float32 numpy: a NaN stays a NaN."""
    x = np.asarray(x, dtype=_F)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), x, np.minimum(np.maximum(x, _F(lo)), _F(hi))).astype(_F)


def head(mu, log_std, eps):
    """The kernel's Gaussian head in float32 numpy, one rounding per operation, in its order (``sac_gauss_head_kernel``'s):

        ls = clamp(log_std, -20, 2); sigma = cephes_expf(ls); s = sigma * eps; x = mu + s; u = clamp(x, -1, 1)
        t = (u - mu) / sigma; term = (-0.5 * (t * t) - ls) - ln(2 pi) / 2; logp = term[:, 0] + term[:, 1]

    ``mu`` (n, 2) the tanh mean, ``log_std`` (2,), ``eps`` (n, 2).  Returns ``(u (n, 2), logp (n,), sigma (2,))``."""
    mu, eps = np.asarray(mu, dtype=_F), np.asarray(eps, dtype=_F)
    ls = tclamp(np.asarray(log_std, dtype=_F).reshape(-1), LOG_STD_MIN, LOG_STD_MAX)
    if mu.ndim != 2 or mu.shape[1] != ACT_DIM or eps.shape != mu.shape or ls.shape != (ACT_DIM,):
        raise ValueError("mu and eps must have shape (n, 2) and log_std 2 elements")
    sigma = cephes_expf(ls)
    with np.errstate(all="ignore"):
        s = sigma * eps
        x = mu + s
        u = tclamp(x, -1.0, 1.0)
        t = (u - mu) / sigma
        tt = t * t
        term = ((_F(-0.5) * tt) - ls) - HALF_LN_2PI
        logp = term[:, 0] + term[:, 1]
    return u.astype(_F), logp.astype(_F), sigma


def random_actions(seed: int, env_ids, counter: int) -> np.ndarray:
    """float32 (len(env_ids), 2) in (-1, 1): column c takes word c of Philox4x32-10((g, counter_lo, counter_hi, RANDOM_TAG), key =
    seed) as u = ((w >> 9) + 0.5) * 2**-23, and the action is -1 + 2 * u: a product and a sum, each rounded to float32."""
    ids = np.asarray(env_ids, dtype=np.int64).reshape(-1, 1)
    w = philox4x32(ids.astype(np.uint64) & np.uint64(_MASK), int(counter) & _MASK, (int(counter) >> 32) & _MASK, np.uint64(RANDOM_TAG),
                   int(seed) & _MASK, (int(seed) >> 32) & _MASK)
    u = unit_uniform(np.concatenate(w[:ACT_DIM], axis=1)).astype(_F)
    return (_F(-1.0) + (_F(2.0) * u).astype(_F)).astype(_F)


def action_normals(seed: int, env_ids, counter: int) -> np.ndarray:
    """float64 eps (len(env_ids), 2): the Box-Muller of ``rollout.standard_normals`` under ACTION_TAG."""
    return standard_normals(seed, env_ids, counter, ACT_DIM, tag=ACTION_TAG)


class _SacModeMixin:
    """The mode of a step and the checks the two implementations share."""

    def _init_sac(self, random_timesteps: int) -> None:
        if self.A != ACT_DIM:
            raise ValueError("the memory must hold 2-wide actions (the SAC parameter vector fixes log_std at 2 floats)")
        self.random_timesteps = int(random_timesteps)

    def mode(self, timestep: int, deterministic: bool = False) -> int:
        """MEAN for evaluation; else RANDOM while ``timestep < random_timesteps`` (skrl), then SAMPLE."""
        if deterministic:
            return MEAN
        return RANDOM if int(timestep) < self.random_timesteps else SAMPLE

    @staticmethod
    def _batch(batch_size):
        if batch_size is not None and int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        return None if batch_size is None else int(batch_size)


# ------------------------------------------------------------------------------------------------------------------ the spec
class TorchSACCollector(_SacModeMixin, TorchTD3Collector):
    """The specification, in torch / numpy.  ``actor``: any callable (n, 965) -> (n, 2) returning the tanh mean; ``log_std``: a
    tensor of 2 floats, read at every ``act``.  ``begin`` is ``TorchTD3Collector``'s."""

    def __init__(self, actor, log_std, memory: ReplayMemory, seed: int = 42, env_id_offset: int = 0, random_timesteps: int = 0,
                 state_scaler=None):
        super().__init__(actor, memory, seed, env_id_offset, 0.0, (-1.0, 1.0), state_scaler)
        self._init_sac(random_timesteps)
        self.log_std = log_std
        self.last: dict = {}

    def draws(self, counter: int | None = None) -> np.ndarray:
        """float64 eps (n, 2) of ``counter`` (default: the next call's)."""
        ids = self.env_id_offset + np.arange(self.n, dtype=np.int64)
        return action_normals(self.seed, ids, self.counter if counter is None else counter)

    @torch.no_grad()
    def act(self, timestep: int, deterministic: bool = False, eps=None) -> torch.Tensor:
        """``eps`` (n, 2) float32, SAMPLE only: use these standard normals instead of the float64 Box-Muller's (a test feeds the
        device's own draws, so that no transcendental of the draw enters the comparison).  ``last`` keeps the step's mean, eps, logp
        and sigma (those the mode produces)."""
        m = self.memory
        mode = self.mode(timestep, deterministic)
        dev = m.actions.device
        if mode == RANDOM:
            ids = self.env_id_offset + np.arange(self.n, dtype=np.int64)
            a = torch.from_numpy(random_actions(self.seed, ids, self.counter)).to(dev)
            self.last = {}
        else:
            mean = self.actor(self._states())
            a, self.last = mean, {"mean": mean}
            if mode == SAMPLE:
                e = self.draws().astype(_F) if eps is None else eps.detach().cpu().numpy().astype(_F)
                u, logp, sigma = head(mean.detach().cpu().numpy(), self.log_std.detach().cpu().numpy(), e)
                a = torch.from_numpy(u).to(dev)
                self.last.update(eps=torch.from_numpy(e), logp=torch.from_numpy(logp), sigma=torch.from_numpy(sigma))
        m.actions[m.memory_index] = a
        self.counter += 1
        return a

    @torch.no_grad()
    def record(self, raw_obs, rew, terminated, batch_size: int | None = None):
        """``TorchTD3Collector.record``; with ``batch_size`` returns ``(idx, eps)``: the int64 row indices and the update's float32
        standard normals (batch_size, 4) of the same counter (columns 0:2 for s', 2:4 for s).  Else ``None``."""
        batch_size, counter = self._batch(batch_size), self.counter
        idx = super().record(raw_obs, rew, terminated, batch_size)
        if batch_size is None:
            return None
        eps = torch.from_numpy(smooth_normals(self.seed, counter, batch_size, 4).astype(_F)).to(self.memory.device)
        return idx, eps


# ---------------------------------------------------------------------------------------------------------------- the kernels
def default_hparams() -> "_lib.SacCollectHparams":
    return _fused.default_hparams(_lib.SacCollectHparams, "rover_sac_collect_default_hparams")


def collect_act(actor, log_std, rows: torch.Tensor, counter: int, hp: "_lib.SacCollectHparams", act_out: torch.Tensor,
                env_act_out: torch.Tensor, *, mean_out=None, eps_out=None, logp_out=None, sigma_out=None) -> None:
    """One ``rover_sac_collect_act`` launch on the current stream over the already-sanitised ``rows`` (n, 965); ``log_std`` (RANDOM and
    MEAN do not read it) and the outputs left ``None`` are passed as NULL."""
    n = int(rows.shape[0])
    wide = (("act_out", act_out), ("env_act_out", env_act_out), ("mean_out", mean_out), ("eps_out", eps_out))
    narrow = (("log_std", log_std, ACT_DIM), ("logp_out", logp_out, n), ("sigma_out", sigma_out, ACT_DIM))
    _launch_act("rover_sac_collect_act", actor, rows, ACT_DIM, wide, narrow, C.byref(actor.desc), actor.packed.data_ptr(),
                actor.n_copies, ptr(log_std), C.byref(hp), C.c_uint64(int(counter)), rows.data_ptr(), n, ptr(mean_out),
                act_out.data_ptr(), env_act_out.data_ptr(), ptr(eps_out), ptr(logp_out), ptr(sigma_out))


def collect_record(raw: torch.Tensor, ring_slot: torch.Tensor, hp: "_lib.SacCollectHparams", counter: int = 0, *, rew=None,
                   terminated=None, rew_out=None, term_out=None, ring_pos_entry=None, ring_pos_value: int = 0, idx_out=None,
                   mem_rows: int = 0, eps_out=None) -> None:
    """One ``rover_sac_collect_record`` launch on the current stream; every argument left ``None`` is passed as NULL.  The batch is
    ``idx_out``'s length, or ``eps_out``'s (batch, 4) when no indices are asked for."""
    n = int(raw.shape[0])
    batch = 0
    if idx_out is not None:
        batch = int(idx_out.numel())
    if eps_out is not None:
        if eps_out.dtype != torch.float32 or not eps_out.is_contiguous() or eps_out.dim() != 2 or eps_out.shape[1] != 4:
            raise ValueError("eps_out must be a contiguous float32 tensor of shape (batch, 4)")
        if idx_out is not None and int(eps_out.shape[0]) != batch:
            raise ValueError("idx_out and eps_out must hold the same batch")
        batch = int(eps_out.shape[0])
    launch("rover_sac_collect_record", raw.device, raw.data_ptr(), n, ring_slot.data_ptr(), ptr(rew), ptr(terminated), ptr(rew_out),
           ptr(term_out), ptr(ring_pos_entry), int(ring_pos_value), ptr(idx_out), batch, int(mem_rows), ptr(eps_out), C.byref(hp),
           C.c_uint64(int(counter)))


class SACCollector(_SacModeMixin, _FusedCollector):
    """The fused collector: ``actor`` is a tanh ``RoverNet`` (reference architecture, two outputs), ``log_std`` a float32 cuda tensor
    of 2 floats and ``memory`` a ``ReplayMemory`` on the same device, all held BY REFERENCE -- with ``FusedSAC.actor`` and
    ``FusedSAC.log_std`` the collector always sees the trainer's current parameters.  ``act`` returns a buffer the next call
    overwrites, ``record`` likewise (one index / draw buffer pair per batch size): ``begin`` and ``record`` are the fused base
    class's, ``record`` returning ``(idx, eps)``.  ``state_scaler`` as ``TD3Collector``'s: the actor reads ``scaler.forward`` of the
    cursor slot (one more launch, in every mode), the ring keeps the raw rows.
    """

    _NAME = "SACCollector"
    _DRAWS = True

    def __init__(self, actor, log_std: torch.Tensor, memory: ReplayMemory, seed: int = 42, env_id_offset: int = 0,
                 random_timesteps: int = 0, state_scaler=None):
        super().__init__(memory, seed, env_id_offset, 0.0, (-1.0, 1.0), state_scaler)
        self._init_sac(random_timesteps)
        self._bind(actor)
        self.log_std = log_std
        if actor.out_dim != ACT_DIM:
            raise ValueError("the actor must have 2 outputs")
        f32_cuda("log_std", log_std, actor.packed.device)
        if log_std.numel() != ACT_DIM:
            raise ValueError("log_std must hold 2 floats")

    def hparams(self, mode: int = SAMPLE) -> "_lib.SacCollectHparams":
        hp = self._seeded(default_hparams())
        hp.mode = int(mode)
        return hp

    def _record(self, raw, ring_slot, counter=0, idx=None, eps=None, **transition) -> None:
        collect_record(raw, ring_slot, self.hparams(), counter, idx_out=idx, eps_out=eps, **transition)

    @torch.no_grad()
    def act(self, timestep: int, deterministic: bool = False, mean_out=None, eps_out=None, logp_out=None,
            sigma_out=None) -> torch.Tensor:
        """One launch in the mode of ``timestep`` on the ring's cursor slot.  Fills the memory's action slot and returns the actions
        for ``env.step``.  Advances the counter by one."""
        m = self.memory
        collect_act(self.actor, self.log_std, self._states(), self.counter, self.hparams(self.mode(timestep, deterministic)),
                    m.actions[m.memory_index], self._env_act, mean_out=mean_out, eps_out=eps_out, logp_out=logp_out,
                    sigma_out=sigma_out)
        self.counter += 1
        return self._env_act
