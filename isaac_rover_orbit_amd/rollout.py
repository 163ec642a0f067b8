"""The on-policy half of a rollout as library code: sanitise, act, sample, log-prob, record (include/rover_rollout.h).

Per env step a PPO / TRPO trainer needs, around ``env.step`` (the reference: ``agent.act`` + ``record_transition``,
rover_envs/utils/skrl_utils.py:114-135): the sanitised observation rows in the rollout buffer, the policy mean, the value, a
Gaussian action, the action the env takes (clipped, models.py:66) and the log-probability.  ``RolloutCollector`` does all of it in
ONE HIP launch (``rover_rollout_act``) and records reward / done in a second, small one; it owns the ``(T, n, ...)`` tensors
``obs``, ``actions``, ``mean``, ``logp``, ``val``, ``rew`` and ``done`` that ``FusedPPO.update``, ``FusedPPO.gae`` and ``FusedTRPO``
take as they are.

The action noise is counter-based, like every draw of the env: Philox4x32-10 keyed by the seed, indexed by (global env
id, step counter, action pair).  Its values do not depend on tensor shapes or on how the envs are split over ranks, and the
checkpoint is ``{seed, counter, env_id_offset}``.

``TorchRollout`` is the same interface in plain torch / numpy: the specification of the kernel (Philox restated in integer
arithmetic, Box-Muller in float64), and it runs on the CPU with any callables as networks.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _fused, _lib
from ._fused import f32_cuda, holds, launch, ptr

ROLLOUT_TAG = 0x524F4C00          # "ROL\0": word 3 of the Philox counter, | action pair (the env's draws have word 3 in {0, 1, 2})
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
HALF_LOG_2PI = 0.9189385332
FLT_MAX = float(np.finfo(np.float32).max)
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------- the draws (spec)
def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on integer arrays (broadcast against each other): four uint32 words per input, as uint64 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & np.uint64(_MASK) for x in (c0, c1, c2, c3, k0, k1)])
    m = np.uint64(_MASK)
    s = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2     # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ k0, p1 & m, (p0 >> s) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(_W0)) & m, (k1 + np.uint64(_W1)) & m
    return c0, c1, c2, c3


def rollout_counter(env_ids, counter: int, pair, tag: int = ROLLOUT_TAG):
    """The Philox input (c0, c1, c2, c3) of global env id(s) ``env_ids``, step ``counter`` and action pair(s) ``pair``; ``tag`` is
    the stream's word 3 (the lift collector draws under a tag of its own)."""
    return (np.asarray(env_ids, dtype=np.uint64) & np.uint64(_MASK), np.uint64(int(counter) & _MASK),
            np.uint64((int(counter) >> 32) & _MASK), np.uint64(int(tag) & _MASK) | np.asarray(pair, dtype=np.uint64))


def unit_uniform(w):
    """((w >> 9) + 0.5) * 2**-23 of a 32-bit word: 24 significant bits, so exact in fp32 (and float64), strictly inside (0, 1)."""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def standard_normals(seed: int, env_ids, counter: int, width: int, tag: int = ROLLOUT_TAG) -> np.ndarray:
    """eps (len(env_ids), width) in float64: Box-Muller on the exact uniforms, columns 2p / 2p + 1 = cosine / sine branch of pair p."""
    ids = np.asarray(env_ids, dtype=np.int64).reshape(-1, 1)
    pairs = np.arange((width + 1) // 2, dtype=np.int64).reshape(1, -1)
    w0, w1, _, _ = philox4x32(*rollout_counter(ids, counter, pairs, tag), int(seed) & _MASK, (int(seed) >> 32) & _MASK)
    u1, u2 = unit_uniform(w0), unit_uniform(w1)
    rho = np.sqrt(-2.0 * np.log(u1))
    eps = np.stack([rho * np.cos(2.0 * np.pi * u2), rho * np.sin(2.0 * np.pi * u2)], axis=-1).reshape(ids.shape[0], -1)
    return eps[:, :width]


class _RolloutBase:
    """Buffers, counter and checkpoint shared by the two implementations."""

    def __init__(self, log_std, num_envs: int, horizon: int, seed: int, env_id_offset: int, clip_actions: bool, device):
        self.n, self.T = int(num_envs), int(horizon)
        if self.n < 1 or self.T < 1:
            raise ValueError("num_envs and horizon must be >= 1")
        self.log_std = log_std
        self.A = int(log_std.numel())
        self.seed, self.env_id_offset, self.clip_actions = int(seed), int(env_id_offset), bool(clip_actions)
        self.counter = 0
        self.device = torch.device(device)
        f = dict(dtype=torch.float32, device=self.device)
        self.obs = torch.zeros(self.T, self.n, 965, **f)
        self.actions = torch.zeros(self.T, self.n, self.A, **f)      # `act` is the method
        self.mean = torch.zeros(self.T, self.n, self.A, **f)
        self.logp, self.val, self.rew, self.done = (torch.zeros(self.T, self.n, **f) for _ in range(4))

    def state_dict(self) -> dict:
        """The checkpoint of the action noise: the counter, not a generator state."""
        return {"seed": self.seed, "counter": self.counter, "env_id_offset": self.env_id_offset}

    def load_state_dict(self, sd: dict) -> None:
        self.seed, self.counter, self.env_id_offset = int(sd["seed"]), int(sd["counter"]), int(sd["env_id_offset"])

    def _raw(self, raw_obs) -> torch.Tensor:
        if isinstance(raw_obs, dict):
            raw_obs = raw_obs["policy"]
        if raw_obs.dim() != 2 or tuple(raw_obs.shape) != (self.n, 965) or raw_obs.dtype != torch.float32:
            raise ValueError(f"raw_obs must be a float32 tensor of shape ({self.n}, 965)")
        if raw_obs.device != self.device:
            raise ValueError(f"raw_obs must live on {self.device}")
        return raw_obs.contiguous()


# ------------------------------------------------------------------------------------------------------------------ the spec
class TorchRollout(_RolloutBase):
    """The specification, in plain torch / numpy.  ``actor`` / ``critic``: any callables (n, 965) -> (n, A) / (n, 1)."""

    def __init__(self, actor, critic, log_std, num_envs: int, horizon: int, seed: int = 42, env_id_offset: int = 0,
                 clip_actions: bool = True, device="cpu"):
        super().__init__(log_std, num_envs, horizon, seed, env_id_offset, clip_actions, device)
        self.actor, self.critic = actor, critic

    @staticmethod
    def sanitise(raw_obs: torch.Tensor) -> torch.Tensor:
        return torch.nan_to_num(raw_obs, nan=0.0, posinf=FLT_MAX, neginf=0.0)

    def draws(self, counter: int | None = None) -> np.ndarray:
        """float64 eps (n, A) of step ``counter`` (default: the next one)."""
        ids = self.env_id_offset + np.arange(self.n, dtype=np.int64)
        return standard_normals(self.seed, ids, self.counter if counter is None else counter, self.A)

    @torch.no_grad()
    def act(self, t: int, raw_obs) -> torch.Tensor:
        o = self.sanitise(self._raw(raw_obs))
        mean, val = self.actor(o), self.critic(o).reshape(self.n)
        eps = torch.from_numpy(self.draws().astype(np.float32)).to(self.device)
        ls = self.log_std.detach().to(self.device).clamp(LOG_STD_MIN, LOG_STD_MAX)
        std = ls.exp()
        a = mean + std * eps
        self.obs[t], self.mean[t], self.val[t], self.actions[t] = o, mean, val, a
        self.logp[t] = (-0.5 * ((a - mean) / std) ** 2 - ls - HALF_LOG_2PI).sum(1)
        self.counter += 1
        return a.clamp(-1.0, 1.0) if self.clip_actions else a

    @torch.no_grad()
    def record(self, t: int, rew, terminated, truncated, rewards_shaper_scale=None, time_limit_bootstrap: bool = False,
               discount: float = 0.99) -> None:
        if rewards_shaper_scale is not None or time_limit_bootstrap:
            from .ppo_skrl import shape_rewards
            rew = shape_rewards(rew, self.val[t], truncated, 1.0 if rewards_shaper_scale is None else rewards_shaper_scale, discount,
                                time_limit_bootstrap)
        self.rew[t] = rew
        self.done[t] = (terminated.bool() | truncated.bool()).float()

    @torch.no_grad()
    def last_value(self, raw_obs) -> torch.Tensor:
        return self.critic(self.sanitise(self._raw(raw_obs))).reshape(self.n)


# ---------------------------------------------------------------------------------------------------------------- the kernels
def rollout_act(actor, critic, log_std: torch.Tensor, raw_obs: torch.Tensor, counter: int, hp: "_lib.RolloutHparams", *,
                obs_out=None, mean_out=None, val_out=None, act_out=None, env_act_out=None, logp_out=None, eps_out=None):
    """One ``rover_rollout_act`` launch on the current stream; ``mean_out`` / ``val_out`` are allocated when not given, every other
    output left ``None`` is passed as NULL (not computed).  Returns ``(mean_out, val_out)``."""
    n = int(raw_obs.shape[0])
    f = dict(dtype=torch.float32, device=raw_obs.device)
    if mean_out is None:
        mean_out = torch.empty(n, actor.out_dim, **f)
    if val_out is None:
        val_out = torch.empty(n, critic.out_dim, **f)
    if actor.n_copies != critic.n_copies:
        raise ValueError("actor and critic must hold the same number of packed replicas")
    A = actor.out_dim
    for name, t, shape in (("raw_obs", raw_obs, (n, 965)), ("log_std", log_std, A), ("obs_out", obs_out, (n, 965)),
                           ("mean_out", mean_out, (n, A)), ("val_out", val_out, (n, critic.out_dim)), ("act_out", act_out, (n, A)),
                           ("env_act_out", env_act_out, (n, A)), ("logp_out", logp_out, (n,)), ("eps_out", eps_out, (n, A))):
        f32_cuda(name, t, actor.packed.device, "the networks' device")
        holds(name, t, shape)
    launch("rover_rollout_act", raw_obs.device, C.byref(actor.desc), actor.packed.data_ptr(), C.byref(critic.desc),
           critic.packed.data_ptr(), actor.n_copies, C.byref(hp), C.c_uint64(int(counter)), raw_obs.data_ptr(), n, log_std.data_ptr(),
           ptr(obs_out), mean_out.data_ptr(), val_out.data_ptr(), ptr(act_out), ptr(env_act_out), ptr(logp_out), ptr(eps_out))
    return mean_out, val_out


def default_hparams() -> "_lib.RolloutHparams":
    return _fused.default_hparams(_lib.RolloutHparams, "rover_rollout_default_hparams")


def _transition(n: int, device, *named) -> None:
    """Refuses a reward / flag / output tensor, given as (name, tensor, dtypes), that is not ``n`` contiguous values on ``device``."""
    for name, x, dts in named:
        if not x.is_cuda or x.dtype not in dts or not x.is_contiguous() or x.numel() != n or x.device != device:
            raise ValueError(f"{name} must be a contiguous {dts[0]} cuda tensor of {n} elements")


_FLAG = (torch.bool, torch.uint8)


class RolloutCollector(_RolloutBase):
    """The fused rollout: ``actor`` / ``critic`` are ``RoverNet`` s and ``log_std`` a device tensor, all held BY REFERENCE -- with
    ``FusedPPO.actor``, ``FusedPPO.critic`` and ``FusedPPO.log_std`` the collector always sees the trainer's current parameters.

        env_actions = collector.act(t, obs)            # one launch: slot t of obs / mean / val / actions / logp
        obs, rew, term, trunc, info = env.step(env_actions)
        collector.record(t, rew, term, trunc)           # one small launch: slot t of rew / done
    """

    def __init__(self, actor, critic, log_std: torch.Tensor, num_envs: int, horizon: int, seed: int = 42, env_id_offset: int = 0,
                 clip_actions: bool = True):
        _fused.require_gpu("RolloutCollector", "TorchRollout is the CPU specification")
        if not log_std.is_cuda or log_std.dtype != torch.float32:
            raise ValueError("log_std must be a float32 cuda tensor (a view into the trainer's parameters works as it is)")
        super().__init__(log_std, num_envs, horizon, seed, env_id_offset, clip_actions, actor.packed.device)
        self._lib = _lib.load()
        self.actor, self.critic = actor, critic
        if actor.out_dim != self.A or actor.out_dim > 16:
            raise ValueError("log_std must hold one value per action column (at most 16)")
        self._env_act = torch.zeros(self.n, self.A, dtype=torch.float32, device=self.device)
        self._last_mean = torch.zeros(self.n, self.A, dtype=torch.float32, device=self.device)
        self._last_val = torch.zeros(self.n, critic.out_dim, dtype=torch.float32, device=self.device)
        if critic.out_dim != 1:
            raise ValueError("the critic must have one output")

    def hparams(self) -> "_lib.RolloutHparams":
        hp = _fused.seeded(default_hparams(), self.seed, self.env_id_offset)
        hp.clip_actions = int(self.clip_actions)
        return hp

    @torch.no_grad()
    def act(self, t: int, raw_obs) -> torch.Tensor:
        """Fills slot ``t`` from the env's raw observation rows and returns the actions for ``env.step`` (a buffer the next call
        overwrites).  Advances the counter by one."""
        raw = self._raw(raw_obs)
        rollout_act(self.actor, self.critic, self.log_std, raw, self.counter, self.hparams(), obs_out=self.obs[t],
                    mean_out=self.mean[t], val_out=self.val[t].unsqueeze(1), act_out=self.actions[t], env_act_out=self._env_act,
                    logp_out=self.logp[t])
        self.counter += 1
        return self._env_act

    @torch.no_grad()
    def record(self, t: int, rew: torch.Tensor, terminated: torch.Tensor, truncated: torch.Tensor, rewards_shaper_scale=None,
               time_limit_bootstrap: bool = False, discount: float = 0.99) -> None:
        """Slot ``t`` of ``rew`` / ``done``.  ``rewards_shaper_scale`` (a float; the reference's ``reward_shaper_function``) and
        ``time_limit_bootstrap`` (skrl: ``rewards += discount * values * truncated``, with slot ``t`` of ``val``, the value of the
        pre-step states) take ``rover_rollout_record_shaped``; both at their defaults: the plain launch."""
        _transition(self.n, self.device, ("rew", rew, (torch.float32,)), ("terminated", terminated, _FLAG), ("truncated", truncated, _FLAG))
        if rewards_shaper_scale is not None or time_limit_bootstrap:
            scale = 1.0 if rewards_shaper_scale is None else float(rewards_shaper_scale)
            launch("rover_rollout_record_shaped", self.device, rew.data_ptr(), terminated.data_ptr(), truncated.data_ptr(),
                   self.val[t].data_ptr(), self.n, scale, float(discount), int(bool(time_limit_bootstrap)), self.rew[t].data_ptr(),
                   self.done[t].data_ptr())
            return
        launch("rover_rollout_record", self.device, rew.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), self.n,
               self.rew[t].data_ptr(), self.done[t].data_ptr())

    @torch.no_grad()
    def last_value(self, raw_obs) -> torch.Tensor:
        """The bootstrap value of the rows after the last step: no draw, the counter stays."""
        rollout_act(self.actor, self.critic, self.log_std, self._raw(raw_obs), self.counter, self.hparams(),
                    mean_out=self._last_mean, val_out=self._last_val)
        return self._last_val[:, 0]
