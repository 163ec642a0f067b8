"""The on-policy half of a lift-task rollout as library code: scale, act, sample, log-prob, record (include/rover_lift_rollout.h).

Per env step a PPO trainer of ``FrankaCubeLift-v0`` needs, around ``env.step``: the raw observation rows in the rollout buffer (the
update standardises them itself), the policy mean and the value of the STANDARDISED rows, the value taken back through the value
scaler, a Gaussian action (not clipped: skrl_ppo_cfg.yaml ``clip_actions: False``) and its log-probability; afterwards the scaled
reward, the done flag and the tally of the episodes that ended.  ``LiftRolloutCollector`` does the first part in ONE HIP launch
(``rover_lift_rollout_act``) and the second in a small one (``rover_lift_rollout_record``); it owns the ``(T, n, ...)`` tensors
``obs``, ``actions``, ``mean``, ``logp``, ``val``, ``rew`` and ``done`` that ``FusedLiftPPO.gae`` and ``FusedLiftPPO.update`` take as
they are, and reads the trainer's parameters, ``log_std`` and both scaler blocks by reference.

The action noise is counter-based, as the rover collector's (``rollout.py``): Philox4x32-10 keyed by the seed, indexed by (global
env id, step counter, action pair) under the tag ``LIFT_ROLLOUT_TAG``; the checkpoint is ``{seed, counter, env_id_offset}``.

``TorchLiftRollout`` is the same interface in plain torch / numpy: the specification of the kernels, and it runs on the CPU with
any callables as networks and scalers.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _fused, _lib
from ._fused import f32_cuda, holds, launch, ptr
from .lift_ppo import OBS_DIM
from .rollout import _FLAG, _transition, standard_normals

LIFT_ROLLOUT_TAG = 0x4C524F00     # "LRO\0": word 3 of the Philox counter, | action pair (the lift env's draws have word 3 = 0 or 1 + resample index)
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
LOG_WORDS = 9                     # log[0:8]: means / counts of the envs reset in a step, log[8]: their number


class _LiftRolloutBase:
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
        self.obs = torch.zeros(self.T, self.n, OBS_DIM, **f)
        self.actions = torch.zeros(self.T, self.n, self.A, **f)      # `act` is the method
        self.mean = torch.zeros(self.T, self.n, self.A, **f)
        self.logp, self.val, self.rew, self.done = (torch.zeros(self.T, self.n, **f) for _ in range(4))
        self.ep_sum, self.ep_count = torch.zeros(8, **f), torch.zeros((), **f)

    def state_dict(self) -> dict:
        """The checkpoint of the action noise: the counter, not a generator state."""
        return {"seed": self.seed, "counter": self.counter, "env_id_offset": self.env_id_offset}

    def load_state_dict(self, sd: dict) -> None:
        self.seed, self.counter, self.env_id_offset = int(sd["seed"]), int(sd["counter"]), int(sd["env_id_offset"])

    def reset_tally(self) -> None:
        """Zero the episode tally (``ep_sum``, ``ep_count``), e.g. at the start of an iteration."""
        self.ep_sum.zero_()
        self.ep_count.zero_()

    def _rows(self, obs) -> torch.Tensor:
        if isinstance(obs, dict):
            obs = obs["policy"]
        if obs.dim() != 2 or tuple(obs.shape) != (self.n, OBS_DIM) or obs.dtype != torch.float32:
            raise ValueError(f"obs must be a float32 tensor of shape ({self.n}, {OBS_DIM})")
        if obs.device != self.device:
            raise ValueError(f"obs must live on {self.device}")
        return obs.contiguous()


# ------------------------------------------------------------------------------------------------------------------ the spec
class TorchLiftRollout(_LiftRolloutBase):
    """The specification, in plain torch / numpy: what examples/05_train_lift.py does around ``env.step``.  ``actor`` / ``critic``:
    any callables (n, 36) -> (n, A) / (n, 1) on standardised rows; ``state_pre``: rows -> standardised rows; ``value_inv``: critic
    output -> value (``None``: the raw critic output)."""

    def __init__(self, actor, critic, log_std, state_pre, value_inv, num_envs: int, horizon: int, seed: int = 42,
                 env_id_offset: int = 0, clip_actions: bool = False, reward_scale: float = 0.01, device="cpu",
                 log_std_min: float = LOG_STD_MIN, log_std_max: float = LOG_STD_MAX):
        super().__init__(log_std, num_envs, horizon, seed, env_id_offset, clip_actions, device)
        self.actor, self.critic, self.state_pre, self.value_inv = actor, critic, state_pre, value_inv
        self.reward_scale = float(np.float32(reward_scale))
        self.log_std_min, self.log_std_max = float(log_std_min), float(log_std_max)

    def draws(self, counter: int | None = None) -> np.ndarray:
        """float64 eps (n, A) of step ``counter`` (default: the next one)."""
        ids = self.env_id_offset + np.arange(self.n, dtype=np.int64)
        return standard_normals(self.seed, ids, self.counter if counter is None else counter, self.A, tag=LIFT_ROLLOUT_TAG)

    def _value(self, s) -> torch.Tensor:
        v = self.critic(s)
        return (v if self.value_inv is None else self.value_inv(v)).reshape(self.n)

    @torch.no_grad()
    def act(self, t: int, obs, eps: torch.Tensor | None = None) -> torch.Tensor:
        """Fills slot ``t`` and returns the actions for ``env.step``; ``eps`` (n, A) replaces the step's draws when given.
        Advances the counter by one either way."""
        o = self._rows(obs)
        s = self.state_pre(o)
        mean = self.actor(s)
        if eps is None:
            eps = torch.from_numpy(self.draws().astype(np.float32)).to(self.device)
        ls = self.log_std.detach().to(self.device).clamp(self.log_std_min, self.log_std_max)
        std = ls.exp()
        a = mean + std * eps
        self.logp[t] = (-0.5 * ((a - mean) / std) ** 2 - ls - 0.9189385332).sum(-1)      # lift_ppo.gaussian_logp under the window
        self.val[t] = self._value(s)
        self.obs[t], self.mean[t], self.actions[t] = o, mean, a
        self.counter += 1
        return a.clamp(-1.0, 1.0) if self.clip_actions else a

    @torch.no_grad()
    def record(self, t: int, rew, terminated, truncated, log=None) -> None:
        self.rew[t] = rew * self.reward_scale
        self.done[t] = (terminated.bool() | truncated.bool()).float()
        if log is not None:
            k = log[8]                                                # envs reset in this step; log[0:8] are their means
            add = log[0:8] * torch.where(torch.arange(8, device=self.device) < 6, k, 1.0)
            self.ep_sum.copy_(torch.where(k > 0, self.ep_sum + add, self.ep_sum))      # the header's "if k > 0": a zero, negative
            self.ep_count.copy_(torch.where(k > 0, self.ep_count + k, self.ep_count))  # or NaN k moves no bit of the tally

    @torch.no_grad()
    def last_value(self, obs) -> torch.Tensor:
        return self._value(self.state_pre(self._rows(obs)))


# ---------------------------------------------------------------------------------------------------------------- the kernels
def default_hparams() -> "_lib.LiftRolloutHparams":
    return _fused.default_hparams(_lib.LiftRolloutHparams, "rover_lift_rollout_default_hparams")


def lift_rollout_act(actor, critic, log_std: torch.Tensor, obs: torch.Tensor, counter: int, hp: "_lib.LiftRolloutHparams",
                     state_scaler: torch.Tensor, value_scaler: torch.Tensor | None = None, *, obs_out=None, mean_out=None,
                     val_out=None, act_out=None, env_act_out=None, logp_out=None, eps_out=None):
    """One ``rover_lift_rollout_act`` launch on the current stream; ``mean_out`` / ``val_out`` are allocated when not given, every
    other output left ``None`` is passed as NULL (not computed), ``value_scaler=None`` leaves the value raw.  Returns
    ``(mean_out, val_out)``."""
    if obs.dim() != 2 or obs.shape[1] != OBS_DIM:
        raise ValueError(f"obs must be (n, {OBS_DIM})")
    n = int(obs.shape[0])
    f = dict(dtype=torch.float32, device=obs.device)
    if mean_out is None:
        mean_out = torch.empty(n, actor.out_dim, **f)
    if val_out is None:
        val_out = torch.empty(n, 1, **f)
    if actor.n_copies != critic.n_copies:
        raise ValueError("actor and critic must hold the same number of packed replicas")
    A = actor.out_dim
    for name, t, shape in (("obs", obs, (n, OBS_DIM)), ("log_std", log_std, (A,)), ("obs_out", obs_out, (n, OBS_DIM)),
                           ("mean_out", mean_out, (n, A)), ("val_out", val_out, (n, 1)), ("act_out", act_out, (n, A)),
                           ("env_act_out", env_act_out, (n, A)), ("logp_out", logp_out, (n,)), ("eps_out", eps_out, (n, A))):
        f32_cuda(name, t, actor.packed.device, "the networks' device")
        holds(name, t, shape)
    for name, t, w in (("state_scaler", state_scaler, OBS_DIM), ("value_scaler", value_scaler, 1)):
        if t is None:
            continue
        if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != 2 * w + 1 or t.device != obs.device:
            raise ValueError(f"{name} must be a contiguous float64 cuda tensor of {2 * w + 1} values (mean, var, count)")
    launch("rover_lift_rollout_act", obs.device, C.byref(actor.desc), actor.packed.data_ptr(), C.byref(critic.desc),
           critic.packed.data_ptr(), actor.n_copies, C.byref(hp), C.c_uint64(int(counter)), obs.data_ptr(), n, log_std.data_ptr(),
           state_scaler.data_ptr(), ptr(value_scaler), ptr(obs_out), mean_out.data_ptr(), val_out.data_ptr(), ptr(act_out),
           ptr(env_act_out), ptr(logp_out), ptr(eps_out))
    return mean_out, val_out


def lift_rollout_record(rew: torch.Tensor, terminated: torch.Tensor, truncated: torch.Tensor, reward_scale: float,
                        rew_out: torch.Tensor, done_out: torch.Tensor, log=None, ep_sum=None, ep_count=None) -> None:
    """One ``rover_lift_rollout_record`` launch on the current stream (``log=None``: no tally)."""
    n = int(rew.numel())
    dev = rew.device
    _transition(n, dev, ("rew", rew, (torch.float32,)), ("terminated", terminated, _FLAG), ("truncated", truncated, _FLAG),
                ("rew_out", rew_out, (torch.float32,)), ("done_out", done_out, (torch.float32,)))
    if log is not None:
        for name, x, m in (("log", log, LOG_WORDS), ("ep_sum", ep_sum, 8), ("ep_count", ep_count, 1)):
            if x is None or not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() < m or x.device != dev:
                raise ValueError(f"{name} must be a contiguous float32 cuda tensor of at least {m} elements")
    launch("rover_lift_rollout_record", dev, rew.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), n,
           C.c_float(float(reward_scale)), ptr(log), rew_out.data_ptr(), done_out.data_ptr(), ptr(ep_sum) if log is not None else None,
           ptr(ep_count) if log is not None else None)


class LiftRolloutCollector(_LiftRolloutBase):
    """The fused lift rollout on a ``FusedLiftPPO``: its ``actor``, ``critic``, ``log_std``, ``state_scaler`` and ``value_scaler``
    are held BY REFERENCE, so the collector always sees the trainer's current parameters and statistics -- nothing to re-pack.

        env_actions = collector.act(t, obs)                 # one launch: slot t of obs / mean / val / actions / logp
        obs, rew, term, trunc, info = env.step(env_actions)
        collector.record(t, rew, term, trunc, log)           # one small launch: slot t of rew / done, the episode tally
    """

    def __init__(self, trainer, num_envs: int, horizon: int, seed: int = 42, env_id_offset: int = 0, clip_actions: bool = False):
        _fused.require_gpu("LiftRolloutCollector", "TorchLiftRollout is the CPU specification")
        super().__init__(trainer.log_std, num_envs, horizon, seed, env_id_offset, clip_actions, trainer.actor.packed.device)
        self._lib = _lib.load()
        self.trainer = trainer
        self.actor, self.critic = trainer.actor, trainer.critic
        if self.actor.out_dim != self.A or self.A > 16 or self.critic.out_dim != 1:
            raise ValueError("the actor must have one output per log_std value (at most 16) and the critic one output")
        f = dict(dtype=torch.float32, device=self.device)
        self._env_act = torch.zeros(self.n, self.A, **f)
        self._last_mean = torch.zeros(self.n, self.A, **f)
        self._last_val = torch.zeros(self.n, 1, **f)

    @property
    def reward_scale(self) -> float:
        return float(self.trainer.hp.reward_scale)

    def hparams(self) -> "_lib.LiftRolloutHparams":
        hp, th = _fused.seeded(default_hparams(), self.seed, self.env_id_offset), self.trainer.hp
        hp.clip_actions = int(self.clip_actions)
        hp.log_std_min, hp.log_std_max = th.log_std_min, th.log_std_max
        hp.scaler_eps, hp.scaler_clip, hp.reward_scale = th.scaler_eps, th.scaler_clip, th.reward_scale
        return hp

    @torch.no_grad()
    def act(self, t: int, obs) -> torch.Tensor:
        """Fills slot ``t`` from the env's observation rows and returns the actions for ``env.step`` (a buffer the next call
        overwrites).  Advances the counter by one."""
        tr = self.trainer
        lift_rollout_act(self.actor, self.critic, tr.log_std, self._rows(obs), self.counter, self.hparams(), tr.state_scaler,
                         tr.value_scaler, obs_out=self.obs[t], mean_out=self.mean[t], val_out=self.val[t].unsqueeze(1),
                         act_out=self.actions[t], env_act_out=self._env_act, logp_out=self.logp[t])
        self.counter += 1
        return self._env_act

    @torch.no_grad()
    def record(self, t: int, rew: torch.Tensor, terminated: torch.Tensor, truncated: torch.Tensor, log=None) -> None:
        """Slot ``t`` of ``rew`` (scaled by the trainer's ``reward_scale``) and ``done``; with ``log`` (the env's device log
        vector) the episodes that ended in this step are added to ``ep_sum`` / ``ep_count``."""
        if rew.numel() != self.n:
            raise ValueError(f"rew must be a contiguous torch.float32 cuda tensor of {self.n} elements")
        lift_rollout_record(rew, terminated, truncated, self.reward_scale, self.rew[t], self.done[t], log, self.ep_sum, self.ep_count)

    @torch.no_grad()
    def last_value(self, obs) -> torch.Tensor:
        """The bootstrap value of the rows after the last step: no draw, the counter stays."""
        tr = self.trainer
        lift_rollout_act(self.actor, self.critic, tr.log_std, self._rows(obs), self.counter, self.hparams(), tr.state_scaler,
                         tr.value_scaler, mean_out=self._last_mean, val_out=self._last_val)
        return self._last_val[:, 0]
