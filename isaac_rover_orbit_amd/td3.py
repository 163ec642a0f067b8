"""TD3 for the rover's actor and twin critics: the replay memory, the torch spec (skrl 1.1 ``TD3._update``) and the fused HIP
update on the MI355X (C ABI: ``include/rover_td3.h``).

The reference trains TD3 with ``learning/train/td3.py``: ``get_model_double_critic_deterministic`` models, skrl's
``RandomMemory(memory_size = 2 x batch_size)`` and ``rover_td3.yaml``.  skrl is not a dependency here; ``TorchTD3`` restates its
TD3 in torch and each function names the skrl function it follows.  Where skrl's behaviour is stated from memory it is a
hyper-parameter.

Networks: the actor is ``examples/04_train_ppo.py``'s ``Net(2, False)`` (no tanh, no log_std).  The critic is ``Critic``,
Q(s, a) with the action appended to the MLP input -- a deliberate deviation: the reference's ``Critic.compute`` never reads
``taken_actions`` when it has an encoder (models.py:270-276), so its Q ignores the action and skrl's TD3 never changes the
actor.

``ReplayMemory`` keeps one observation ring of ``memory_size + 1`` slots per env: the ``next_states`` of a transition are the
``states`` of the next one (the reference's loop ends every step with ``states.copy_(next_states)``), so the ring holds both
at half of skrl's two-buffer footprint.

``FusedTD3`` runs the update as HIP kernels on one flat device vector ``[actor | critic_1 | critic_2 | padding]`` with a target
vector of the same layout.  ``.actor`` aliases the trainer's actor.  No CPU fallback.
"""
from __future__ import annotations

import copy
import ctypes as C
import itertools
from typing import Mapping

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _fused, _lib
from ._fused import ptr
from .ppo import _layers, pack, unpack

# skrl TD3_DEFAULT_CONFIG with rover_td3.yaml (batch 4096, actor / critic lr 1e-4).  skrl's defaults stated from memory:
# gradient_steps 1, discount 0.99, polyak 0.005, policy_delay 2, smooth_regularization_noise None (clip 0.5),
# exploration noise None (initial_scale 1.0, final_scale 1e-3, timesteps None), random_timesteps = learning_starts = 0,
# grad_norm_clip 0.  Adam's betas / eps are torch's defaults.
HPARAMS = dict(gradient_steps=1, batch_size=4096, discount_factor=0.99, polyak=0.005, actor_learning_rate=1e-4,
               critic_learning_rate=1e-4, policy_delay=2, smooth_regularization_clip=0.5, clip_actions_min=-1.0, clip_actions_max=1.0,
               exploration_initial_scale=1.0, exploration_final_scale=1e-3, exploration_timesteps=None, random_timesteps=0,
               learning_starts=0, grad_norm_clip=0.0)
OBS_DIM, ACT_DIM = 965, 2
CHECKPOINT_KEYS = ("policy", "target_policy", "critic_1", "critic_2", "target_critic_1", "target_critic_2")


class Critic(nn.Module):
    """Q(s, a): encoder 961 -> 80 -> 60 on obs[:, 3:-1] (the reference's one-column-early slice), MLP on
    [obs[:, 0:4], enc, a] 66 -> 256 -> 160 -> 128 -> 1, LeakyReLU(0.01).  State-dict names as ``Net``'s."""

    def __init__(self):
        super().__init__()
        act = nn.LeakyReLU
        self.dense_encoder = nn.Module()
        self.dense_encoder.encoder_layers = nn.ModuleList([nn.Linear(961, 80), act(), nn.Linear(80, 60), act()])
        self.mlp = nn.ModuleList([nn.Linear(66, 256), act(), nn.Linear(256, 160), act(), nn.Linear(160, 128), act(), nn.Linear(128, 1)])

    def forward(self, s, a):
        e = s[:, 3:-1]
        for layer in self.dense_encoder.encoder_layers:
            e = layer(e)
        x = torch.cat([s[:, 0:4], e, a], 1)
        for layer in self.mlp:
            x = layer(x)
        return x


# ---------------------------------------------------------------------------------------------------------------- memory
class ReplayMemory:
    """skrl ``RandomMemory`` semantics on an observation ring.

    Memory slot k (0 .. memory_size) holds actions, rewards and terminated of one ``add``; its states lie in ring slot
    ``ring_pos[k]`` and its next_states in ring slot ``(ring_pos[k] + 1) % (memory_size + 1)``.  ``add`` writes states to the
    ring's cursor slot and next_states to the one after it, then advances the cursor by one, so the ``next_states`` of one
    add are overwritten by the ``states`` of the following add: the two must be equal, as in the reference's loop.  When
    ``states`` is the very tensor passed as the previous ``next_states`` (and unchanged since), that write is skipped.
    Row indices are flat, ``slot * num_envs + env``, as ``RandomMemory.sample`` draws them.
    """

    def __init__(self, memory_size: int, num_envs: int, device="cuda", obs_dim: int = OBS_DIM, act_dim: int = ACT_DIM):
        if memory_size < 1 or num_envs < 1:
            raise ValueError("memory_size and num_envs must be >= 1")
        self.memory_size, self.num_envs, self.slots = int(memory_size), int(num_envs), int(memory_size) + 1
        self.device = torch.device(device)
        self.obs = torch.zeros(self.slots, self.num_envs, obs_dim, device=self.device)
        self.actions = torch.zeros(self.memory_size, self.num_envs, act_dim, device=self.device)
        self.rewards = torch.zeros(self.memory_size, self.num_envs, device=self.device)
        self.terminated = torch.zeros(self.memory_size, self.num_envs, dtype=torch.bool, device=self.device)
        self.ring_pos = torch.zeros(self.memory_size, dtype=torch.int32, device=self.device)
        self.memory_index, self.filled, self.cursor = 0, False, 0
        self._last_next, self._last_version = None, -1

    @staticmethod
    def nbytes(memory_size: int, num_envs: int, obs_dim: int = OBS_DIM, act_dim: int = ACT_DIM) -> int:
        """Device bytes of a memory of this size (the ring dominates: (memory_size + 1) x num_envs x obs_dim floats)."""
        M, N = int(memory_size), int(num_envs)
        return 4 * (M + 1) * N * obs_dim + 4 * M * N * act_dim + 4 * M * N + M * N + 4 * M

    @staticmethod
    def two_buffer_nbytes(memory_size: int, num_envs: int, obs_dim: int = OBS_DIM, act_dim: int = ACT_DIM) -> int:
        """skrl's RandomMemory: states and next_states stored apart."""
        M, N = int(memory_size), int(num_envs)
        return 2 * 4 * M * N * obs_dim + 4 * M * N * act_dim + 4 * M * N + M * N

    def __len__(self) -> int:
        return (self.memory_size if self.filled else self.memory_index) * self.num_envs

    def add(self, states, actions, rewards, next_states, terminated):
        """RandomMemory.add_samples of one env step (every env)."""
        N, k, w = self.num_envs, self.memory_index, self.cursor
        if not (states is self._last_next and states._version == self._last_version):
            self.obs[w].copy_(states.reshape(N, -1))
        nw = (w + 1) % self.slots
        self.obs[nw].copy_(next_states.reshape(N, -1))
        self.actions[k].copy_(actions.reshape(N, -1))
        self.rewards[k].copy_(rewards.reshape(N))
        self.terminated[k].copy_(terminated.reshape(N))
        self.ring_pos[k] = w
        self.cursor = nw
        self.memory_index += 1
        if self.memory_index >= self.memory_size:
            self.memory_index, self.filled = 0, True
        self._last_next, self._last_version = next_states, next_states._version

    def sample_indices(self, batch_size: int, generator: torch.Generator | None = None) -> torch.Tensor:
        """RandomMemory.sample's indices: randint(0, len(memory)) with replacement (int64, on the memory's device)."""
        n = len(self)
        if n == 0:
            raise ValueError("the memory is empty")
        return torch.randint(0, n, (int(batch_size),), device=self.device, generator=generator)

    def gather(self, idx: torch.Tensor):
        """(states, actions, rewards (B, 1), next_states, terminated (B, 1)) of flat row indices, as the sampled tensors of
        skrl's memory."""
        idx = idx.to(self.device, torch.int64)
        k, e = idx // self.num_envs, idx % self.num_envs
        pos = self.ring_pos[k].long()
        s = self.obs[pos, e]
        s2 = self.obs[(pos + 1) % self.slots, e]
        a = self.actions.view(-1, self.actions.shape[-1])[idx]
        r = self.rewards.view(-1)[idx].unsqueeze(1)
        t = self.terminated.view(-1)[idx].unsqueeze(1)
        return s, a, r, s2, t


# ---------------------------------------------------------------------------------------------------------------- torch spec
def update_parameters(target: nn.Module, model: nn.Module, polyak: float):
    """skrl Model.update_parameters: exact copy at polyak 1, else t.mul_(1 - polyak); t.add_(polyak * p)."""
    with torch.no_grad():
        for t, p in zip(target.parameters(), model.parameters()):
            if polyak == 1:
                t.copy_(p)
            else:
                t.mul_(1 - polyak)
                t.add_(polyak * p)


def exploration_scale(timestep: int, timesteps: int, initial_scale: float = 1.0, final_scale: float = 1e-3,
                      exploration_timesteps: int | None = None) -> float | None:
    """skrl TD3.act's linear noise scale; None once the schedule has ended (no noise is added then)."""
    horizon = timesteps if exploration_timesteps is None else exploration_timesteps
    if timestep > horizon:
        return None
    return (1 - timestep / horizon) * (initial_scale - final_scale) + final_scale


def explore(actions: torch.Tensor, noise: torch.Tensor, scale: float | None, clip_min=-1.0, clip_max=1.0) -> torch.Tensor:
    """skrl TD3.act: actions + scale * noise, clamped to the action range; unchanged once the schedule has ended."""
    if scale is None:
        return actions
    return (actions + noise * scale).clamp(clip_min, clip_max)


class TorchTD3:
    """skrl TD3._update in torch autograd on ``Net(2, False)`` and two ``Critic``; any dtype (the tests run float64)."""

    def __init__(self, policy: nn.Module, critic_1: nn.Module, critic_2: nn.Module, **hparams):
        self.hp = dict(HPARAMS)
        for k, v in hparams.items():
            if k not in self.hp:
                raise TypeError(f"unknown hyper-parameter {k!r}")
            self.hp[k] = v
        self.policy, self.critic_1, self.critic_2 = policy, critic_1, critic_2
        # skrl TD3.__init__: target models start as update_parameters(model, polyak=1), an exact copy
        self.target_policy, self.target_critic_1, self.target_critic_2 = (copy.deepcopy(m) for m in (policy, critic_1, critic_2))
        for m in (self.target_policy, self.target_critic_1, self.target_critic_2):
            m.requires_grad_(False)
        self.policy_optimizer = torch.optim.Adam(self.policy.parameters(), lr=self.hp["actor_learning_rate"])
        self.critic_optimizer = torch.optim.Adam(itertools.chain(self.critic_1.parameters(), self.critic_2.parameters()),
                                                 lr=self.hp["critic_learning_rate"])
        self.critic_update_counter = 0

    @property
    def dtype(self):
        return next(self.policy.parameters()).dtype

    def act(self, states):
        """TD3.act without exploration noise: pi(s)."""
        with torch.no_grad():
            return self.policy(states)

    def target_values(self, next_states, rewards, terminated, noise=None):
        """y = r + gamma * !terminated * min(tq1, tq2) with the (optionally smoothed) target action."""
        hp = self.hp
        with torch.no_grad():
            next_actions = self.target_policy(next_states)
            if noise is not None:
                noises = torch.clamp(noise.to(next_actions.dtype), min=-hp["smooth_regularization_clip"], max=hp["smooth_regularization_clip"])
                next_actions.add_(noises)
                next_actions.clamp_(min=hp["clip_actions_min"], max=hp["clip_actions_max"])
            target_q1_values = self.target_critic_1(next_states, next_actions)
            target_q2_values = self.target_critic_2(next_states, next_actions)
            target_q_values = torch.min(target_q1_values, target_q2_values)
            return rewards + hp["discount_factor"] * terminated.logical_not() * target_q_values

    def critic_step(self, states, actions, rewards, next_states, terminated, noise=None) -> dict:
        """The critic half of one gradient step: y, the twin-critic MSE, one Adam step over both critics."""
        target_values = self.target_values(next_states, rewards, terminated, noise)
        critic_1_values = self.critic_1(states, actions)
        critic_2_values = self.critic_2(states, actions)
        critic_loss = (F.mse_loss(critic_1_values, target_values) + F.mse_loss(critic_2_values, target_values)) / 2
        self.critic_optimizer.zero_grad()
        critic_loss.backward()
        if self.hp["grad_norm_clip"] > 0:
            nn.utils.clip_grad_norm_(itertools.chain(self.critic_1.parameters(), self.critic_2.parameters()), self.hp["grad_norm_clip"])
        self.critic_optimizer.step()
        return {"critic_loss": float(critic_loss.detach()), "q1_mean": float(critic_1_values.detach().mean()),
                "q2_mean": float(critic_2_values.detach().mean()), "y_mean": float(target_values.mean()), "y": target_values}

    def actor_step(self, states) -> dict:
        """The delayed actor step: -mean q1(s, pi(s)) with the critic_1 just updated, one Adam step on the actor."""
        actions = self.policy(states)
        critic_values = self.critic_1(states, actions)
        policy_loss = -critic_values.mean()
        self.policy_optimizer.zero_grad()
        policy_loss.backward()
        if self.hp["grad_norm_clip"] > 0:
            nn.utils.clip_grad_norm_(self.policy.parameters(), self.hp["grad_norm_clip"])
        self.policy_optimizer.step()
        return {"policy_loss": float(policy_loss.detach())}

    def polyak(self):
        """The three target updates that follow an actor step."""
        for t, m in ((self.target_critic_1, self.critic_1), (self.target_critic_2, self.critic_2), (self.target_policy, self.policy)):
            update_parameters(t, m, self.hp["polyak"])

    def update(self, memory: ReplayMemory, idx: torch.Tensor, noise: torch.Tensor | None = None) -> dict:
        """One gradient step (gradient_steps = 1) on the rows ``idx`` of ``memory``; the actor and the targets step on every
        ``policy_delay``-th call."""
        dt = self.dtype
        s, a, r, s2, t = memory.gather(idx)
        st = self.critic_step(s.to(dt), a.to(dt), r.to(dt), s2.to(dt), t, noise)
        st.pop("y")
        self.critic_update_counter += 1
        st["actor_stepped"] = not self.critic_update_counter % self.hp["policy_delay"]
        if st["actor_stepped"]:
            st.update(self.actor_step(s.to(dt)))
            self.polyak()
        return st

    def checkpoint(self) -> dict:
        return {k: getattr(self, k).state_dict() for k in CHECKPOINT_KEYS}


# ---------------------------------------------------------------------------------------------------------------- fused
def default_hparams() -> "_lib.Td3Hparams":
    return _fused.default_hparams(_lib.Td3Hparams, "rover_td3_default_hparams")


def critic_desc() -> "_lib.PolicyDesc":
    d = _lib.PolicyDesc()
    _lib.check(_lib.load().rover_td3_critic_desc(C.byref(d)), "rover_td3_critic_desc")
    return d


def pack_critic(sd: Mapping[str, torch.Tensor]):
    """(descriptor, packed host array) of a ``Critic`` state_dict (``rover_td3_critic_pack``)."""
    ws, bs, n_enc = _layers(sd)
    if n_enc != 2 or len(ws) != 6:
        raise ValueError("not a Critic state_dict (2 encoder and 4 MLP layers)")
    desc = critic_desc()
    return desc, _fused.pack_layers(desc, ws, bs, "rover_td3_critic_pack")


STAT_KEYS = ("critic_loss", "q1_mean", "q2_mean", "y_mean", "policy_loss", "critic_step", "actor_step", "bad_index")


class FusedTD3(_fused.FusedOffPolicy):
    """TD3 trainer state on the GPU: parameters, targets, Adam moments and the device state struct (rover_td3_state).

    ``update`` runs one gradient step without a host synchronisation; ``stats`` reads the state (one synchronisation).  The
    host counts the critic steps and runs the actor step and Polyak on every ``policy_delay``-th one.

    Hyper-parameters are float32 in the C struct.  ``polyak`` is bit-identical to torch's fp32 ``t.mul_(1 - tau); t.add_(tau * p)``
    for ``tau = float(numpy.float32(polyak))``; that is skrl's result with the double ``polyak`` whenever
    ``float32(1 - polyak) == float32(1 - float32(polyak))`` (0.005, 0.05, 0.25: yes; 0.9, 0.99, 0.995, 0.999: no, see
    ``rover_td3_polyak`` in rover_td3.h).  ``polyak = 1`` copies the parameters.
    """

    _STATE, _WORKSPACE, _PARAM_FLOATS = _lib.Td3State, "rover_td3_workspace_bytes", "rover_td3_param_floats"
    _RUNS = "the reference actor (Net(2, False)) and td3.Critic only (rover_td3.h)"
    _unpack = staticmethod(unpack)

    def __init__(self, policy_sd: Mapping[str, torch.Tensor], critic_1_sd: Mapping[str, torch.Tensor],
                 critic_2_sd: Mapping[str, torch.Tensor], target_policy_sd=None, target_critic_1_sd=None, target_critic_2_sd=None,
                 policy_delay: int = 2, device="cuda", n_copies: int = 4, **hparams):
        super().__init__(default_hparams, hparams, device, n_copies)
        self.policy_delay, self.critic_updates = int(policy_delay), 0
        pa, pc1, pc2 = self._networks(pack(policy_sd, "none"), pack_critic(critic_1_sd), pack_critic(critic_2_sd))
        tp = pack(target_policy_sd, "none")[1] if target_policy_sd is not None else pa
        t1 = pack_critic(target_critic_1_sd)[1] if target_critic_1_sd is not None else pc1
        t2 = pack_critic(target_critic_2_sd)[1] if target_critic_2_sd is not None else pc2
        self._alloc(self._vector(pa, pc1, pc2))
        self.target = torch.from_numpy(self._vector(tp, t1, t2)).to(self.device)
        self.state = torch.zeros(C.sizeof(_lib.Td3State) // 4, dtype=torch.int32, device=self.device)

    def _vector(self, pa, pc1, pc2) -> np.ndarray:
        return np.concatenate([pa, pc1, pc2, np.zeros(self.P - pa.size - pc1.size - pc2.size, np.float32)])

    @staticmethod
    def _checkpoint_args(ck):
        """skrl TD3 checkpoint ``{"policy", "target_policy", "critic_1", "critic_2", "target_critic_1", "target_critic_2"}``;
        missing target entries start as copies."""
        return (ck["policy"], ck["critic_1"], ck["critic_2"], ck.get("target_policy"), ck.get("target_critic_1"),
                ck.get("target_critic_2"))

    # ---- views
    def state_dict(self) -> dict:
        """skrl TD3 checkpoint keys; state dicts that ``Net(2, False)`` / ``Critic`` load (float32 CPU tensors)."""
        p, t = self.unvector(self.params), self.unvector(self.target)
        return {"policy": p["policy"], "target_policy": t["policy"], "critic_1": p["critic_1"], "critic_2": p["critic_2"],
                "target_critic_1": t["critic_1"], "target_critic_2": t["critic_2"]}

    # ---- kernels
    def critic_step(self, memory: ReplayMemory, idx: torch.Tensor, noise: torch.Tensor | None = None, y_out: torch.Tensor | None = None):
        n = self._sample(memory, idx)
        if noise is not None and (not noise.is_cuda or noise.dtype != torch.float32 or not noise.is_contiguous()
                                  or noise.numel() != 2 * n):
            raise ValueError("noise must be a contiguous float32 cuda tensor of (n, 2)")
        _lib.check(self._lib.rover_td3_critic_step(
            C.byref(self.desc_a), C.byref(self.desc_c), C.byref(self.hp), self.params.data_ptr(), self.target.data_ptr(),
            self.grad.data_ptr(), self.adam_m.data_ptr(), self.adam_v.data_ptr(), memory.obs.data_ptr(), memory.slots, memory.num_envs,
            memory.ring_pos.data_ptr(), memory.actions.data_ptr(), memory.rewards.data_ptr(), memory.terminated.data_ptr(),
            idx.data_ptr(), n, len(memory), ptr(noise), self.ws.data_ptr(), self.ws.numel(), self.state.data_ptr(),
            self._out(y_out, n, "y_out"), self._stream()), "rover_td3_critic_step")
        self.critic_updates += 1

    def actor_step(self, memory: ReplayMemory, idx: torch.Tensor, dact_out: torch.Tensor | None = None):
        n = self._sample(memory, idx)
        _lib.check(self._lib.rover_td3_actor_step(
            C.byref(self.desc_a), C.byref(self.desc_c), C.byref(self.hp), self.params.data_ptr(), self.grad.data_ptr(),
            self.adam_m.data_ptr(), self.adam_v.data_ptr(), memory.obs.data_ptr(), memory.slots, memory.num_envs,
            memory.ring_pos.data_ptr(), idx.data_ptr(), n, len(memory), self.ws.data_ptr(), self.ws.numel(), self.state.data_ptr(),
            self.rep_a.data_ptr(), self.n_copies, self._out(dact_out, 2 * n, "dact_out"), self._stream()), "rover_td3_actor_step")

    def polyak(self):
        _lib.check(self._lib.rover_td3_polyak(C.byref(self.hp), self.target.data_ptr(), self.params.data_ptr(), self.P, self._stream()),
                   "rover_td3_polyak")

    def update(self, memory: ReplayMemory, idx: torch.Tensor, noise: torch.Tensor | None = None) -> bool:
        """One gradient step on rows ``idx`` of ``memory`` (no host synchronisation); returns whether the actor stepped."""
        self.critic_step(memory, idx, noise)
        if self.critic_updates % self.policy_delay:
            return False
        self.actor_step(memory, idx)
        self.polyak()
        return True
