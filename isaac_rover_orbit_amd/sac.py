"""SAC for the rover's Gaussian actor, twin critics and learned entropy coefficient: the torch spec (skrl 1.1 ``SAC._update``)
and the fused HIP update on the MI355X (C ABI: ``include/rover_sac.h``).

The reference trains SAC with ``learning/train/sac.py`` and ``rover_sac.yaml``.  Its ``sac.py`` builds a ``DeterministicActor``,
which returns no log-probability, while ``rover_sac.yaml``'s ``policy`` block describes a Gaussian model (``clip_log_std``,
``min_log_std: -20``, ``max_log_std: 2``, tanh output): the reference's ``GaussianNeuralNetwork``, the actor PPO and TRPO train
here.  This module builds that evident intent: the policy is ``examples/04_train_ppo.py``'s
``Net(2, True)`` (tanh on the mean, a ``log_std_parameter`` of 2, initial 0), the critics are ``td3.Critic`` Q(s, a), the
memory is ``td3.ReplayMemory``.  There is no target policy.

skrl is not a dependency here; ``TorchSAC`` restates its SAC in torch and each function names the skrl function it follows.
Where skrl's behaviour is stated from memory it is a hyper-parameter.  The standard normal draws are GIVEN to ``update``
(``eps`` of shape (B, 4): columns 0:2 for s', columns 2:4 for s), so the spec and the fused path see the same sample.

``FusedSAC`` runs the update as HIP kernels on one flat device vector
``[actor | critic_1 | critic_2 | log_std (2 + 2 pad) | log_alpha (1 + 3 pad) | padding]`` and a target vector
``[critic_1 | critic_2]``.  ``.actor`` aliases the trainer's actor, ``.log_std`` is a view into the vector.  No CPU fallback.
"""
from __future__ import annotations

import copy
import ctypes as C
import itertools
import math
from typing import Mapping

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _fused, _lib
from .ppo import pack, unpack
from .td3 import ACT_DIM, ReplayMemory, pack_critic, update_parameters

# skrl SAC_DEFAULT_CONFIG with rover_sac.yaml (batch 4096, actor / critic lr 1e-4).  skrl's defaults stated from memory:
# gradient_steps 1, discount 0.99, polyak 0.005, entropy_learning_rate 5e-3 (rover_sac.yaml), learn_entropy True,
# initial_entropy_value 0.2, target_entropy None (minus the action width), random_timesteps = learning_starts = 0,
# grad_norm_clip 0.  Adam's betas / eps are torch's defaults.
HPARAMS = dict(gradient_steps=1, batch_size=4096, discount_factor=0.99, polyak=0.005, actor_learning_rate=1e-4,
               critic_learning_rate=1e-4, entropy_learning_rate=5e-3, learn_entropy=True, initial_entropy_value=0.2,
               target_entropy=None, random_timesteps=0, learning_starts=0, grad_norm_clip=0.0)
# skrl's SAC checkpoint modules, plus the entropy coefficient's logarithm (skrl does not store it; a resumed run needs it)
CHECKPOINT_KEYS = ("policy", "critic_1", "critic_2", "target_critic_1", "target_critic_2", "log_entropy_coefficient")
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def initial_log_alpha(value: float = HPARAMS["initial_entropy_value"], dtype=torch.float32) -> torch.Tensor:
    """log(float32(initial_entropy_value)) as a 0-dim tensor (skrl: torch.log(torch.ones(1) * initial_entropy_value))."""
    return torch.log(torch.tensor(float(np.float32(value)), dtype=dtype))


def gaussian_act(mu: torch.Tensor, log_std_parameter: torch.Tensor, eps: torch.Tensor):
    """skrl GaussianMixin.act (clip_actions, clip_log_std in [-20, 2], reduction "sum") on a given draw: the clamped rsample
    ``u`` and the log-probability (B, 1) of the CLAMPED action."""
    ls = log_std_parameter.clamp(LOG_STD_MIN, LOG_STD_MAX)
    sigma = ls.exp()
    x = mu + sigma * eps                                    # Normal(mu, sigma).rsample()
    u = x.clamp(-1.0, 1.0)
    logp = (-0.5 * ((u - mu) / sigma) ** 2 - ls - HALF_LOG_2PI).sum(1, keepdim=True)
    return u, logp


def gaussian_head_backward(mu, log_std_parameter, eps, g, alpha, log_alpha=None, target_entropy=-2.0):
    """The closed form the fused policy step's Gaussian head implements (include/rover_sac.h), stated in torch.

    ``mu`` (B, 2) the tanh mean, ``eps`` (B, 2) the draw, ``g`` (B, 2) = d min(q1, q2) / du (torch.min's backward: weight 1 on
    the smaller critic, 0.5 each on a tie), ``alpha`` the entropy coefficient.  With p = 1[-1 <= x <= 1] and t = (u - mu) / sigma:

        dL/dmu = (alpha t / sigma (1 - p) - p g) / B
        dL/dls = (alpha (t^2 - 1 - p t eps) - p g sigma eps) / B
        dL/dz6 = dL/dmu (1 - mu^2)
        dL/dlog_std_parameter = sum_rows dL/dls 1[-20 <= param <= 2]
        dL_ent/dlog_alpha = -mean(logp + target_entropy)

    Returns a dict of those plus ``u`` and ``logp`` (B,)."""
    B = mu.shape[0]
    ls = log_std_parameter.clamp(LOG_STD_MIN, LOG_STD_MAX)
    sigma = ls.exp()
    x = mu + sigma * eps
    u = x.clamp(-1.0, 1.0)
    p = ((x >= -1.0) & (x <= 1.0)).to(mu.dtype)
    t = (u - mu) / sigma
    logp = (-0.5 * t ** 2 - ls - HALF_LOG_2PI).sum(1)
    dmu = (alpha * t / sigma * (1 - p) - p * g) / B
    dls = (alpha * (t * t - 1 - p * t * eps) - p * g * sigma * eps) / B
    mask = ((log_std_parameter >= LOG_STD_MIN) & (log_std_parameter <= LOG_STD_MAX)).to(mu.dtype)
    return {"u": u, "logp": logp, "dmu": dmu, "dls": dls, "dz6": dmu * (1 - mu * mu), "dlog_std": dls.sum(0) * mask,
            "dlog_alpha": -(logp + target_entropy).mean()}


# ---------------------------------------------------------------------------------------------------------------- torch spec
class TorchSAC:
    """skrl SAC._update in torch autograd on ``Net(2, True)`` and two ``td3.Critic``; any dtype (the tests run float64)."""

    def __init__(self, policy: nn.Module, critic_1: nn.Module, critic_2: nn.Module, log_entropy_coefficient=None, **hparams):
        self.hp = dict(HPARAMS)
        for k, v in hparams.items():
            if k not in self.hp:
                raise TypeError(f"unknown hyper-parameter {k!r}")
            self.hp[k] = v
        self.policy, self.critic_1, self.critic_2 = policy, critic_1, critic_2
        # skrl SAC.__init__: target models start as update_parameters(model, polyak=1), an exact copy
        self.target_critic_1, self.target_critic_2 = copy.deepcopy(critic_1), copy.deepcopy(critic_2)
        for m in (self.target_critic_1, self.target_critic_2):
            m.requires_grad_(False)
        dt, dev = self.dtype, next(policy.parameters()).device
        self.target_entropy = -float(ACT_DIM) if self.hp["target_entropy"] is None else float(self.hp["target_entropy"])
        la = initial_log_alpha(self.hp["initial_entropy_value"], dt) if log_entropy_coefficient is None \
            else torch.as_tensor(log_entropy_coefficient).detach().reshape(()).to(dt)
        self.log_entropy_coefficient = la.to(dev).clone().requires_grad_(True)
        self.entropy_coefficient = self.log_entropy_coefficient.detach().exp()
        self.policy_optimizer = torch.optim.Adam(self.policy.parameters(), lr=self.hp["actor_learning_rate"])
        self.critic_optimizer = torch.optim.Adam(itertools.chain(self.critic_1.parameters(), self.critic_2.parameters()),
                                                 lr=self.hp["critic_learning_rate"])
        self.entropy_optimizer = torch.optim.Adam([self.log_entropy_coefficient], lr=self.hp["entropy_learning_rate"])

    @property
    def dtype(self):
        return next(self.policy.parameters()).dtype

    def act(self, states, eps):
        """GaussianMixin.act on a given draw: (clamped action, log-probability (B, 1))."""
        return gaussian_act(self.policy(states), self.policy.log_std_parameter, eps.to(self.dtype))

    def target_values(self, next_states, rewards, terminated, eps):
        """y = r + gamma * !terminated * (min(tq1, tq2) - alpha * logp') at the action sampled for s'."""
        with torch.no_grad():
            next_actions, next_log_prob = self.act(next_states, eps)
            target_q1_values = self.target_critic_1(next_states, next_actions)
            target_q2_values = self.target_critic_2(next_states, next_actions)
            target_q_values = torch.min(target_q1_values, target_q2_values) - self.entropy_coefficient * next_log_prob
            return rewards + self.hp["discount_factor"] * terminated.logical_not() * target_q_values

    def critic_step(self, states, actions, rewards, next_states, terminated, eps) -> dict:
        """The critic part of one gradient step: y, the twin-critic MSE, one Adam step over both critics."""
        target_values = self.target_values(next_states, rewards, terminated, eps)
        critic_1_values = self.critic_1(states, actions)
        critic_2_values = self.critic_2(states, actions)
        critic_loss = (F.mse_loss(critic_1_values, target_values) + F.mse_loss(critic_2_values, target_values)) / 2
        self.critic_optimizer.zero_grad()
        critic_loss.backward()
        self.critic_optimizer.step()
        return {"critic_loss": float(critic_loss.detach()), "q1_mean": float(critic_1_values.detach().mean()),
                "q2_mean": float(critic_2_values.detach().mean()), "y_mean": float(target_values.mean()), "y": target_values}

    def policy_loss(self, states, eps):
        """(policy_loss, actions, log_prob): mean(alpha * logp - min(q1(s, u), q2(s, u)))."""
        actions, log_prob = self.act(states, eps)
        critic_1_values = self.critic_1(states, actions)
        critic_2_values = self.critic_2(states, actions)
        loss = (self.entropy_coefficient * log_prob - torch.min(critic_1_values, critic_2_values)).mean()
        return loss, actions, log_prob

    def policy_step(self, states, eps) -> dict:
        """The policy step with the critics just updated, then the entropy step (both with the alpha from before it)."""
        policy_loss, _, log_prob = self.policy_loss(states, eps)
        self.policy_optimizer.zero_grad()
        self.critic_optimizer.zero_grad()
        policy_loss.backward()
        self.policy_optimizer.step()
        st = {"policy_loss": float(policy_loss.detach()), "logp_mean": float(log_prob.detach().mean()),
              "alpha": float(self.entropy_coefficient)}
        if self.hp["learn_entropy"]:
            entropy_loss = -(self.log_entropy_coefficient * (log_prob + self.target_entropy).detach()).mean()
            self.entropy_optimizer.zero_grad()
            entropy_loss.backward()
            self.entropy_optimizer.step()
            self.entropy_coefficient = self.log_entropy_coefficient.detach().exp()
            st["entropy_loss"] = float(entropy_loss.detach())
        return st

    def polyak(self):
        """The two target updates that end a gradient step."""
        for t, m in ((self.target_critic_1, self.critic_1), (self.target_critic_2, self.critic_2)):
            update_parameters(t, m, self.hp["polyak"])

    def update(self, memory: ReplayMemory, idx: torch.Tensor, eps: torch.Tensor) -> dict:
        """One gradient step (gradient_steps = 1) on the rows ``idx`` of ``memory`` with the draws ``eps`` (B, 4)."""
        dt = self.dtype
        s, a, r, s2, t = memory.gather(idx)
        st = self.critic_step(s.to(dt), a.to(dt), r.to(dt), s2.to(dt), t, eps[:, 0:2])
        st.pop("y")
        st.update(self.policy_step(s.to(dt), eps[:, 2:4]))
        self.polyak()
        return st

    def checkpoint(self) -> dict:
        ck = {k: getattr(self, k).state_dict() for k in CHECKPOINT_KEYS[:-1]}
        ck["log_entropy_coefficient"] = self.log_entropy_coefficient.detach().reshape(1).clone()
        return ck

    @classmethod
    def from_checkpoint(cls, ck, policy: nn.Module, critic_1: nn.Module, critic_2: nn.Module, **hparams) -> "TorchSAC":
        """Loads a checkpoint (a path or the dict) into fresh modules; missing target entries start as copies."""
        if isinstance(ck, str):                 # the specification keeps its own loading
            ck = torch.load(ck, map_location="cpu", weights_only=False)
        policy.load_state_dict(ck["policy"]); critic_1.load_state_dict(ck["critic_1"]); critic_2.load_state_dict(ck["critic_2"])
        spec = cls(policy, critic_1, critic_2, log_entropy_coefficient=ck.get("log_entropy_coefficient"), **hparams)
        for k in ("target_critic_1", "target_critic_2"):
            if ck.get(k) is not None:
                getattr(spec, k).load_state_dict(ck[k])
        return spec


# ---------------------------------------------------------------------------------------------------------------- fused
def default_hparams() -> "_lib.SacHparams":
    return _fused.default_hparams(_lib.SacHparams, "rover_sac_default_hparams")


STAT_KEYS = ("critic_loss", "q1_mean", "q2_mean", "y_mean", "policy_loss", "entropy_loss", "logp_mean", "alpha", "critic_step",
             "actor_step", "entropy_step", "bad_index")
TAIL = 8             # log_std (2 + 2 pad), log_alpha (1 + 3 pad)


class FusedSAC(_fused.FusedOffPolicy):
    """SAC trainer state on the GPU: parameters, target critics, Adam moments and the device state struct (rover_sac_state).

    ``update`` runs one gradient step without a host synchronisation; ``stats`` reads the state (one synchronisation).  The
    entropy coefficient is formed on the device from ``log_alpha`` in the parameter vector.

    Hyper-parameters are float32 in the C struct (``gamma``, ``polyak``, ``actor_lr``, ``critic_lr``, ``entropy_lr``, ``beta1``,
    ``beta2``, ``eps``, ``target_entropy``, ``learn_entropy``).  ``polyak`` follows ``td3.FusedTD3``'s note on float32 taus.
    """

    _STATE, _WORKSPACE, _PARAM_FLOATS = _lib.SacState, "rover_sac_workspace_bytes", "rover_sac_param_floats"
    _RUNS = "the reference's Gaussian actor (Net(2, True)) and td3.Critic only (rover_sac.h)"
    _unpack = staticmethod(unpack)

    def __init__(self, policy_sd: Mapping[str, torch.Tensor], critic_1_sd: Mapping[str, torch.Tensor],
                 critic_2_sd: Mapping[str, torch.Tensor], target_critic_1_sd=None, target_critic_2_sd=None,
                 log_entropy_coefficient=None, device="cuda", n_copies: int = 4, **hparams):
        super().__init__(default_hparams, hparams, device, n_copies, convert={"learn_entropy": lambda v: int(bool(v))})
        if "log_std_parameter" not in policy_sd:
            raise ValueError("the policy state_dict has no log_std_parameter (SAC trains the Gaussian actor, Net(2, True))")
        pa, pc1, pc2 = self._networks(pack(policy_sd, "tanh"), pack_critic(critic_1_sd), pack_critic(critic_2_sd))
        self.tail = self.n_a + 2 * self.n_c
        log_std = torch.as_tensor(policy_sd["log_std_parameter"]).detach().cpu().numpy().astype(np.float32).reshape(-1)
        if log_std.size != ACT_DIM:
            raise ValueError("log_std_parameter must hold 2 floats")
        if log_entropy_coefficient is None:
            la = np.float32(initial_log_alpha().item())
        else:
            la = np.float32(torch.as_tensor(log_entropy_coefficient).detach().cpu().reshape(-1)[0].item())
        tail = np.zeros(self.P - self.tail, np.float32)
        tail[0:2], tail[4] = log_std, la
        self._alloc(np.concatenate([pa, pc1, pc2, tail]))
        t1 = pack_critic(target_critic_1_sd)[1] if target_critic_1_sd is not None else pc1
        t2 = pack_critic(target_critic_2_sd)[1] if target_critic_2_sd is not None else pc2
        self.target = torch.from_numpy(np.concatenate([t1, t2])).to(self.device)
        self.state = torch.zeros(C.sizeof(_lib.SacState) // 4, dtype=torch.int32, device=self.device)
        self.log_std = self.params[self.tail:self.tail + ACT_DIM]
        self.log_alpha = self.params[self.tail + 4:self.tail + 5]

    @staticmethod
    def _checkpoint_args(ck):
        """A checkpoint with ``CHECKPOINT_KEYS``; missing target entries start as copies, a missing ``log_entropy_coefficient`` as
        log(initial_entropy_value)."""
        return (ck["policy"], ck["critic_1"], ck["critic_2"], ck.get("target_critic_1"), ck.get("target_critic_2"),
                ck.get("log_entropy_coefficient"))

    # ---- views
    def blocks(self, vec: torch.Tensor) -> dict:
        """The slices of a vector in the parameter layout (or, for the target vector, its two critic blocks)."""
        a, c = self.n_a, self.n_c
        if vec.numel() == 2 * c:
            return {"critic_1": vec[:c], "critic_2": vec[c:2 * c]}
        return {**super().blocks(vec), "log_std": vec[self.tail:self.tail + ACT_DIM], "log_alpha": vec[self.tail + 4:self.tail + 5]}

    def unvector(self, vec: torch.Tensor) -> dict:
        """state_dict-shaped float32 CPU tensors of each block of a vector in either layout; the policy's entry holds
        ``log_std_parameter``, ``log_entropy_coefficient`` is a 1-element tensor."""
        out = super().unvector(vec)
        if "policy" in out:
            b = self.blocks(vec)
            out["policy"]["log_std_parameter"] = b["log_std"].detach().cpu().clone()
            out["log_entropy_coefficient"] = b["log_alpha"].detach().cpu().clone()
        return out

    def state_dict(self) -> dict:
        """``CHECKPOINT_KEYS``; state dicts that ``Net(2, True)`` / ``Critic`` load (float32 CPU tensors)."""
        p, t = self.unvector(self.params), self.unvector(self.target)
        return {"policy": p["policy"], "critic_1": p["critic_1"], "critic_2": p["critic_2"], "target_critic_1": t["critic_1"],
                "target_critic_2": t["critic_2"], "log_entropy_coefficient": p["log_entropy_coefficient"]}

    # ---- kernels
    def _sample(self, memory: ReplayMemory, idx: torch.Tensor, eps: torch.Tensor) -> int:
        n = super()._sample(memory, idx)
        if (not torch.is_tensor(eps) or eps.device != self.params.device or eps.dtype != torch.float32 or not eps.is_contiguous()
                or eps.dim() != 2 or tuple(eps.shape) != (n, 4)):
            raise ValueError("eps must be a contiguous float32 cuda tensor of (n, 4) on the memory's device")
        return n

    def critic_step(self, memory: ReplayMemory, idx: torch.Tensor, eps: torch.Tensor, y_out: torch.Tensor | None = None):
        n = self._sample(memory, idx, eps)
        _lib.check(self._lib.rover_sac_critic_step(
            C.byref(self.desc_a), C.byref(self.desc_c), C.byref(self.hp), self.params.data_ptr(), self.target.data_ptr(),
            self.grad.data_ptr(), self.adam_m.data_ptr(), self.adam_v.data_ptr(), memory.obs.data_ptr(), memory.slots, memory.num_envs,
            memory.ring_pos.data_ptr(), memory.actions.data_ptr(), memory.rewards.data_ptr(), memory.terminated.data_ptr(),
            idx.data_ptr(), n, len(memory), eps.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.state.data_ptr(),
            self._out(y_out, n, "y_out"), self._stream()), "rover_sac_critic_step")

    def policy_step(self, memory: ReplayMemory, idx: torch.Tensor, eps: torch.Tensor, u_out: torch.Tensor | None = None,
                    logp_out: torch.Tensor | None = None, dmean_out: torch.Tensor | None = None):
        n = self._sample(memory, idx, eps)
        _lib.check(self._lib.rover_sac_policy_step(
            C.byref(self.desc_a), C.byref(self.desc_c), C.byref(self.hp), self.params.data_ptr(), self.grad.data_ptr(),
            self.adam_m.data_ptr(), self.adam_v.data_ptr(), memory.obs.data_ptr(), memory.slots, memory.num_envs,
            memory.ring_pos.data_ptr(), idx.data_ptr(), n, len(memory), eps.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            self.state.data_ptr(), self.rep_a.data_ptr(), self.n_copies, self._out(u_out, 2 * n, "u_out"),
            self._out(logp_out, n, "logp_out"), self._out(dmean_out, 2 * n, "dmean_out"), self._stream()), "rover_sac_policy_step")

    def polyak(self):
        _lib.check(self._lib.rover_sac_polyak(C.byref(self.desc_a), C.byref(self.desc_c), C.byref(self.hp), self.target.data_ptr(),
                                              self.params.data_ptr(), self._stream()), "rover_sac_polyak")

    def update(self, memory: ReplayMemory, idx: torch.Tensor, eps: torch.Tensor):
        """One gradient step on rows ``idx`` of ``memory`` with the draws ``eps`` (n, 4); no host synchronisation."""
        self.critic_step(memory, idx, eps)
        self.policy_step(memory, idx, eps)
        self.polyak()
