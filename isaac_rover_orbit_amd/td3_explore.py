"""TD3's exploration switches on top of the transition collector (include/rover_td3_explore.h).

``td3_collect`` covers skrl's ``TD3.act`` at the defaults of ``rover_td3.yaml``.  The explorers here add what a skrl TD3 user can set
besides: Ornstein-Uhlenbeck exploration noise, ``random_timesteps`` of uniform random actions, and counter-based draws of the target
action's smoothing noise.  They subclass the collectors, so ``begin`` / ``record``, the ring, the index stream and the counter are the
collectors' own; ``act`` takes the timestep instead of a scale and picks the mode as skrl's ``TD3.act`` does::

    ex.begin(obs)
    for t in range(timesteps):
        a = ex.act(t, timesteps)                      # t < random_timesteps: uniform in [low, high]; else the actor + noise + clamp
        obs, rew, term, trunc, info = env.step(a)
        idx = ex.record(obs, rew, term, batch_size)
        if t >= learning_starts:
            fused.update(memory, idx, ex.smooth_noise(batch_size, std))   # std > 0: skrl's smooth_regularization_noise

Every draw is Philox4x32-10 under the collector's seed with a word-3 tag of its own (``TAGS``): the random actions are indexed by
(global env id, counter, action column) and the smoothing noise by (batch position, update counter, action column), so neither
depends on tensor shapes or on how the envs are split over ranks.  The checkpoint is the collector's plus ``update_counter`` and the
OU state.

``TorchTD3Explorer`` is the specification in torch / numpy (the numpy Philox of ``rollout.py``, the kernels' operation order in
float32) and runs on the CPU; ``TD3Explorer`` runs the HIP kernels.  skrl is not a dependency: the OU recurrence and ``random_act``
are this project's reading of skrl 1.1.0 and the spec is the contract (the header names the two places where skrl's text may differ
in the last place or in the draw).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _fused, _lib
from ._fused import launch, ptr
from .lift_rollout import LIFT_ROLLOUT_TAG
from .rollout import ROLLOUT_TAG, _MASK, philox4x32, standard_normals, unit_uniform
from .td3 import HPARAMS, ReplayMemory, exploration_scale
from .td3_collect import INDEX_TAG, NOISE_TAG, TD3Collector, TorchTD3Collector, _launch_act

RANDOM_TAG = 0x54335200           # "T3R\0": word 3 of the Philox counter of the random actions, | action quad
SMOOTH_TAG = 0x54334E00           # "T3N\0": ... of the smoothing noise, | action pair
# every word-3 tag of a Philox stream in this repository: the upper 24 bits name the stream, the low 8 carry an action pair or quad
# (the envs' own draws: 0, 1 and 2 there, rover_hip.h)
SAC_ACTION_TAG = 0x53414300       # "SAC\0": the SAC collector's action draws, | action pair (sac_collect.py, rover_sac_collect.h)
SAC_RANDOM_TAG = 0x53415200       # "SAR\0": ... its random steps' uniforms, | action quad
TAGS = {"env": 0, "rollout": ROLLOUT_TAG, "lift_rollout": LIFT_ROLLOUT_TAG, "td3_noise": NOISE_TAG,
        "td3_index": INDEX_TAG, "td3_random": RANDOM_TAG, "td3_smooth": SMOOTH_TAG,
        "sac_action": SAC_ACTION_TAG, "sac_random": SAC_RANDOM_TAG}
OFF, GAUSSIAN, OU, RANDOM = _lib.TD3_EXPLORE_OFF, _lib.TD3_EXPLORE_GAUSSIAN, _lib.TD3_EXPLORE_OU, _lib.TD3_EXPLORE_RANDOM
NOISES = {None: OFF, "none": OFF, "gaussian": GAUSSIAN, "ou": OU}
OU_DEFAULTS = dict(theta=0.15, sigma=0.2, base_scale=1.0)   # skrl OrnsteinUhlenbeckNoise


# ---------------------------------------------------------------------------------------------------------------- the draws (spec)
def random_uniforms(seed: int, env_ids, counter: int, width: int) -> np.ndarray:
    """float32 u (len(env_ids), width) in (0, 1): column c takes word c & 3 of Philox4x32-10((g, counter_lo, counter_hi,
    RANDOM_TAG | c >> 2), key = seed) as ((w >> 9) + 0.5) * 2**-23, exact in float32."""
    ids = np.asarray(env_ids, dtype=np.int64).reshape(-1, 1)
    quads = np.arange((width + 3) // 4, dtype=np.uint64).reshape(1, -1)
    w = philox4x32(ids.astype(np.uint64) & np.uint64(_MASK), int(counter) & _MASK, (int(counter) >> 32) & _MASK,
                   np.uint64(RANDOM_TAG) | quads, int(seed) & _MASK, (int(seed) >> 32) & _MASK)
    words = np.stack(w, axis=-1).reshape(ids.shape[0], -1)[:, :width]
    return unit_uniform(words).astype(np.float32)


def random_actions(seed: int, env_ids, counter: int, width: int, low: float, high: float) -> np.ndarray:
    """float32 low + (high - low) * u: the range once, then a product and a sum, each rounded to float32."""
    low, high = np.float32(low), np.float32(high)
    rng = np.float32(high - low)
    return (low + (rng * random_uniforms(seed, env_ids, counter, width)).astype(np.float32)).astype(np.float32)


def smooth_normals(seed: int, counter: int, batch: int, width: int) -> np.ndarray:
    """float64 eps (batch, width): the Box-Muller of ``rollout.standard_normals`` indexed by the batch position, under SMOOTH_TAG."""
    return standard_normals(seed, np.arange(int(batch)), counter, width, tag=SMOOTH_TAG)


def ou_step(x: np.ndarray, eps: np.ndarray, theta: float, sigma: float, base_scale: float):
    """(x', noise) of one OU step in float32, five separate operations: t = x * theta; x1 = x - t; s = sigma * eps; x' = x1 + s;
    noise = base_scale * x'."""
    f = np.float32
    x, eps = x.astype(f), eps.astype(f)
    t = (x * f(theta)).astype(f)
    x1 = (x - t).astype(f)
    s = (f(sigma) * eps).astype(f)
    xn = (x1 + s).astype(f)
    return xn, (f(base_scale) * xn).astype(f)


def add_noise_clamp(mean: torch.Tensor, noise: torch.Tensor, scale: float, low: float, high: float) -> torch.Tensor:
    """td3.explore's two float32 operations and torch.clamp (a NaN stays NaN)."""
    return (mean + noise * scale).clamp(low, high)


# ---------------------------------------------------------------------------------------------------------------- shared
class _ExplorerMixin:
    """Mode selection, the OU state, the update counter and the checkpoint shared by the two explorers."""

    def _init_explorer(self, noise, random_timesteps, initial_scale, final_scale, exploration_timesteps, ou_theta, ou_sigma,
                       ou_base_scale):
        if noise not in NOISES:
            raise ValueError(f"noise must be one of {sorted(k for k in NOISES if k)} or None")
        self.noise = NOISES[noise]
        self.random_timesteps = int(random_timesteps)
        self.initial_scale, self.final_scale = float(initial_scale), float(final_scale)
        self.exploration_timesteps = exploration_timesteps
        self.ou = (float(ou_theta), float(ou_sigma), float(ou_base_scale))
        self.update_counter = 0
        self.ou_state = torch.zeros(self.n, self.A, dtype=torch.float32, device=self.memory.obs.device)   # skrl starts at 0

    def mode(self, timestep: int, timesteps: int):
        """(mode, scale) of skrl's TD3.act at ``timestep``: RANDOM below random_timesteps, else the configured noise under
        td3.exploration_scale; OFF once that schedule has ended, and for Gaussian noise of std 0 (as the collector)."""
        if timestep < self.random_timesteps:
            return RANDOM, None
        if self.noise == OFF or (self.noise == GAUSSIAN and self.noise_std == 0.0):
            return OFF, None
        scale = exploration_scale(timestep, timesteps, self.initial_scale, self.final_scale, self.exploration_timesteps)
        return (OFF, None) if scale is None else (self.noise, scale)

    def state_dict(self) -> dict:
        """The collector's checkpoint, the counter of the smoothing draws and the OU state (a CPU copy)."""
        return {**super().state_dict(), "update_counter": self.update_counter, "ou_state": self.ou_state.detach().cpu().clone()}

    def load_state_dict(self, sd: dict) -> None:
        super().load_state_dict(sd)
        self.update_counter = int(sd["update_counter"])
        self.ou_state.copy_(sd["ou_state"])

    @staticmethod
    def _smooth_args(batch, std):
        if int(batch) < 1 or not float(std) >= 0.0:
            raise ValueError("batch must be >= 1 and std >= 0")
        return int(batch), float(std)


# ------------------------------------------------------------------------------------------------------------------ the spec
class TorchTD3Explorer(_ExplorerMixin, TorchTD3Collector):
    """The specification, in plain torch / numpy.  ``actor``: any callable (n, 965) -> (n, A)."""

    def __init__(self, actor, memory: ReplayMemory, seed: int = 42, env_id_offset: int = 0, noise=None, noise_std: float = 0.0,
                 clip=(-1.0, 1.0), random_timesteps: int = HPARAMS["random_timesteps"],
                 initial_scale: float = HPARAMS["exploration_initial_scale"], final_scale: float = HPARAMS["exploration_final_scale"],
                 exploration_timesteps=HPARAMS["exploration_timesteps"], ou_theta: float = OU_DEFAULTS["theta"],
                 ou_sigma: float = OU_DEFAULTS["sigma"], ou_base_scale: float = OU_DEFAULTS["base_scale"], state_scaler=None):
        super().__init__(actor, memory, seed, env_id_offset, noise_std, clip, state_scaler)
        self._init_explorer(noise, random_timesteps, initial_scale, final_scale, exploration_timesteps, ou_theta, ou_sigma, ou_base_scale)

    @torch.no_grad()
    def act(self, timestep: int, timesteps: int, eps=None) -> torch.Tensor:
        """``eps`` (n, A) float32, OU only: use these standard normals instead of the float64 Box-Muller's (a test feeds the device's
        own draws, so that no transcendental enters the comparison)."""
        mode, scale = self.mode(timestep, timesteps)
        if mode in (OFF, GAUSSIAN):
            return super().act(scale)                                  # the collector's text: the two modes are the collector's
        m = self.memory
        ids = self.env_id_offset + np.arange(self.n, dtype=np.int64)
        if mode == RANDOM:
            a = torch.from_numpy(random_actions(self.seed, ids, self.counter, self.A, *self.clip)).to(m.actions.device)
        else:
            mean = self.actor(self._states())
            e = self.draws().astype(np.float32) if eps is None else eps.detach().cpu().numpy().astype(np.float32)
            xn, noise = ou_step(self.ou_state.cpu().numpy(), e, *self.ou)
            self.ou_state.copy_(torch.from_numpy(xn))
            a = add_noise_clamp(mean, torch.from_numpy(noise).to(mean.device), float(scale), *self.clip)
        m.actions[m.memory_index] = a
        self.counter += 1
        return a

    def smooth_noise(self, batch: int, std: float) -> torch.Tensor:
        """float32 (batch, A): std * eps of the current update counter, which advances by one."""
        batch, std = self._smooth_args(batch, std)
        eps = smooth_normals(self.seed, self.update_counter, batch, self.A).astype(np.float32)
        self.update_counter += 1
        return torch.from_numpy((np.float32(std) * eps).astype(np.float32)).to(self.memory.obs.device)


# ---------------------------------------------------------------------------------------------------------------- the kernels
def default_hparams() -> "_lib.Td3ExploreHparams":
    return _fused.default_hparams(_lib.Td3ExploreHparams, "rover_td3_explore_default_hparams")


def explore_act(actor, rows: torch.Tensor, counter: int, hp: "_lib.Td3ExploreHparams", act_out: torch.Tensor,
                env_act_out: torch.Tensor, *, ou_state=None, mean_out=None, eps_out=None) -> None:
    """One ``rover_td3_explore_act`` launch on the current stream over the already-sanitised ``rows`` (n, 965); ``ou_state`` /
    ``mean_out`` / ``eps_out`` left ``None`` are passed as NULL."""
    wide = (("act_out", act_out), ("env_act_out", env_act_out), ("ou_state", ou_state), ("mean_out", mean_out), ("eps_out", eps_out))
    _launch_act("rover_td3_explore_act", actor, rows, actor.out_dim, wide, (), C.byref(actor.desc), actor.packed.data_ptr(),
                actor.n_copies, C.byref(hp), C.c_uint64(int(counter)), rows.data_ptr(), int(rows.shape[0]), ptr(ou_state),
                ptr(mean_out), act_out.data_ptr(), env_act_out.data_ptr(), ptr(eps_out))


def smooth_draw(seed: int, counter: int, std: float, out: torch.Tensor) -> torch.Tensor:
    """One ``rover_td3_smooth_draw`` launch on the current stream into ``out`` (n, A), a contiguous float32 cuda tensor."""
    if not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 2:
        raise ValueError("out must be a contiguous float32 cuda tensor of shape (n, A)")
    launch("rover_td3_smooth_draw", out.device, int(seed) & _MASK, (int(seed) >> 32) & _MASK, C.c_uint64(int(counter)), float(std),
           out.data_ptr(), int(out.shape[0]), int(out.shape[1]))
    return out


class TD3Explorer(_ExplorerMixin, TD3Collector):
    """The fused explorer: ``TD3Collector`` with ``act`` on ``rover_td3_explore_act`` and the smoothing draw.  ``act`` and
    ``smooth_noise`` return buffers the next call overwrites (one noise buffer per batch size)."""

    def __init__(self, actor, memory: ReplayMemory, seed: int = 42, env_id_offset: int = 0, noise=None, noise_std: float = 0.0,
                 clip=(-1.0, 1.0), random_timesteps: int = HPARAMS["random_timesteps"],
                 initial_scale: float = HPARAMS["exploration_initial_scale"], final_scale: float = HPARAMS["exploration_final_scale"],
                 exploration_timesteps=HPARAMS["exploration_timesteps"], ou_theta: float = OU_DEFAULTS["theta"],
                 ou_sigma: float = OU_DEFAULTS["sigma"], ou_base_scale: float = OU_DEFAULTS["base_scale"], state_scaler=None):
        super().__init__(actor, memory, seed, env_id_offset, noise_std, clip, state_scaler)
        self._init_explorer(noise, random_timesteps, initial_scale, final_scale, exploration_timesteps, ou_theta, ou_sigma, ou_base_scale)
        self._smooth: dict = {}

    def explore_hparams(self, mode: int, scale: float | None = None) -> "_lib.Td3ExploreHparams":
        hp = self._seeded(default_hparams())
        hp.mode = mode
        hp.noise_std, hp.noise_scale = self.noise_std, 1.0 if scale is None else float(scale)
        hp.ou_theta, hp.ou_sigma, hp.ou_base_scale = self.ou
        hp.action_low, hp.action_high = self.clip
        return hp

    @torch.no_grad()
    def act(self, timestep: int, timesteps: int, mean_out=None, eps_out=None) -> torch.Tensor:
        """One launch in the mode of ``timestep``.  Fills the memory's action slot and returns the actions for ``env.step``.
        Advances the counter by one."""
        m = self.memory
        mode, scale = self.mode(timestep, timesteps)
        explore_act(self.actor, self._states(), self.counter, self.explore_hparams(mode, scale), m.actions[m.memory_index],
                    self._env_act, ou_state=self.ou_state if mode == OU else None, mean_out=mean_out, eps_out=eps_out)
        self.counter += 1
        return self._env_act

    @torch.no_grad()
    def smooth_noise(self, batch: int, std: float) -> torch.Tensor:
        """The ``noise`` argument of ``FusedTD3.update``: float32 (batch, A) on the device, std * eps of the current update counter,
        which advances by one.  The update clips it (``smooth_regularization_clip``)."""
        batch, std = self._smooth_args(batch, std)
        out = self._smooth.get(batch)
        if out is None:
            out = self._smooth[batch] = torch.zeros(batch, self.A, dtype=torch.float32, device=self.memory.obs.device)
        smooth_draw(self.seed, self.update_counter, std, out)
        self.update_counter += 1
        return out
