"""PPO for the lift task (``FrankaCubeLift-v0``): the torch restatement of skrl's PPO that serves as the spec, and the fused HIP
update on the MI355X (C ABI: ``include/rover_lift_train.h``).

The reference trains the lift task with skrl 1.1.0 PPO and ``rover_envs/envs/manipulation/config/franka/agents/skrl_ppo_cfg.yaml``:
networks 36 -> 256 -> 128 -> 64 -> {8, 1} with ELU (skrl ``gaussian_model`` / ``deterministic_model``), a ``RunningStandardScaler``
on states and one on values, rewards x 0.01, value-loss scale 2, gradient-norm clip 1.0, 24 rollouts, 8 epochs, 24 minibatches,
KL-adaptive learning rate and the KL early stop (0.008).  skrl is not a dependency of this project, so the torch code below
restates each formula and names the skrl function it follows; ``FusedLiftPPO`` runs the same update as HIP kernels, and the
GPU tests pin one to the other.  No CPU fallback for the fused path.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping

import torch
import torch.nn as nn

from . import _fused, _lib
from ._fused import ptr
from .policy import RoverNet, make_desc

OBS_DIM, ACT_DIM = 36, 8
HIDDEN = (256, 128, 64)
LIFT_KEY = "net.{}.{}"               # skrl model instantiators: nn.Sequential, Linear at even indices, ELU at odd ones
LOG_STD_KEY = "log_std_parameter"    # skrl GaussianMixin


def default_hparams() -> "_lib.LiftPpoHparams":
    """skrl_ppo_cfg.yaml of the lift task (rover_lift_ppo_default_hparams)."""
    return _fused.default_hparams(_lib.LiftPpoHparams, "rover_lift_ppo_default_hparams")


# ---------------------------------------------------------------------------------------------------------------- torch spec
class LiftMLP(nn.Module):
    """skrl 1.1.0 ``gaussian_model`` (out_dim 8, with ``log_std_parameter``, initial log_std 0, no output activation) or
    ``deterministic_model`` (out_dim 1) with ``hiddens: [256, 128, 64]``, ``hidden_activation: elu`` (skrl_ppo_cfg.yaml)."""

    def __init__(self, out_dim: int, log_std: bool = False):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(OBS_DIM, HIDDEN[0]), nn.ELU(), nn.Linear(HIDDEN[0], HIDDEN[1]), nn.ELU(),
                                 nn.Linear(HIDDEN[1], HIDDEN[2]), nn.ELU(), nn.Linear(HIDDEN[2], out_dim))
        if log_std:
            self.log_std_parameter = nn.Parameter(torch.zeros(out_dim))

    def forward(self, s):
        return self.net(s)


class RunningStandardScaler:
    """skrl 1.1.0 ``skrl.resources.preprocessors.torch.RunningStandardScaler`` (epsilon 1e-8, clip_threshold 5): float64
    running statistics, initial mean 0, variance 1, count 1."""

    def __init__(self, size: int, epsilon: float = 1e-8, clip_threshold: float = 5.0, device="cuda"):
        self.epsilon, self.clip_threshold = float(epsilon), float(clip_threshold)
        self.running_mean = torch.zeros(size, dtype=torch.float64, device=device)
        self.running_variance = torch.ones(size, dtype=torch.float64, device=device)
        self.current_count = torch.ones((), dtype=torch.float64, device=device)

    def _parallel_variance(self, input_mean, input_var, input_count):
        """RunningStandardScaler._parallel_variance: the parallel-variance merge of a batch's mean and unbiased variance."""
        delta = input_mean - self.running_mean
        total_count = self.current_count + input_count
        M2 = (self.running_variance * self.current_count) + (input_var * input_count) \
            + delta ** 2 * self.current_count * input_count / total_count
        self.running_mean = self.running_mean + delta * input_count / total_count
        self.running_variance = M2 / total_count
        self.current_count = total_count

    def __call__(self, x: torch.Tensor, train: bool = False, inverse: bool = False) -> torch.Tensor:
        """RunningStandardScaler._compute (2-D input)."""
        if train:
            self._parallel_variance(torch.mean(x, dim=0), torch.var(x, dim=0), x.shape[0])
        if inverse:
            return torch.sqrt(self.running_variance.float()) * torch.clamp(x, min=-self.clip_threshold, max=self.clip_threshold) \
                + self.running_mean.float()
        return torch.clamp((x - self.running_mean.float()) / (torch.sqrt(self.running_variance.float()) + self.epsilon),
                           min=-self.clip_threshold, max=self.clip_threshold)

    def state_dict(self) -> dict:
        return {"running_mean": self.running_mean.clone(), "running_variance": self.running_variance.clone(),
                "current_count": self.current_count.clone()}

    def load_state_dict(self, sd: Mapping[str, torch.Tensor]):
        self.running_mean = sd["running_mean"].to(self.running_mean).clone()
        self.running_variance = sd["running_variance"].to(self.running_variance).clone()
        self.current_count = torch.as_tensor(sd["current_count"]).to(self.current_count).clone().reshape(())


def gaussian_logp(mean, log_std, a):
    """skrl GaussianMixin.act: log_std clamped to [-20, 2], Normal(mean, exp(log_std)).log_prob(a) summed over the 8 actions
    (written as -0.5 x^2 - log_std - log sqrt(2 pi) with x = (a - mean) / std, as examples/04_train_ppo.py)."""
    ls = log_std.clamp(-20.0, 2.0)
    return (-0.5 * ((a - mean) / ls.exp()) ** 2 - ls - 0.9189385332).sum(-1)


def lift_ppo_loss(policy, value, s, a, old_lp, old_v, ret, adv, clip=0.2, vclip=0.2, vscale=2.0):
    """skrl 1.1.0 PPO._update, one minibatch on STANDARDISED states s: ratio = exp(logp - old_logp);
    policy loss = -min(adv r, adv clip(r, 1 - clip, 1 + clip)).mean(); predicted values clipped to old_v +- vclip
    (clip_predicted_values); value loss = vscale * mse(ret, v); entropy scale 0.  Returns (loss, kl, policy loss, value loss),
    kl = ((r - 1) - log r).mean() without gradient."""
    lp = gaussian_logp(policy(s), policy.log_std_parameter, a)
    ratio = (lp - old_lp).exp()
    with torch.no_grad():
        kl = ((ratio - 1) - (lp - old_lp)).mean()
    pl = -torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv).mean()
    v = value(s).squeeze(1)
    v = old_v + (v - old_v).clamp(-vclip, vclip)
    vl = vscale * ((ret - v) ** 2).mean()
    return pl + vl, kl, pl.detach(), vl.detach()


def gae_torch(rew, done, val, last_v, gamma=0.99, lam=0.95):
    """GAE in examples/04_train_ppo.py's order (= rover_ppo_gae's, bit for bit); done = terminated | truncated."""
    adv = torch.zeros_like(rew)
    gae = torch.zeros_like(last_v)
    for t in reversed(range(rew.shape[0])):
        nv = last_v if t == rew.shape[0] - 1 else val[t + 1]
        nd = 1.0 - done[t]
        delta = rew[t] + gamma * nv * nd - val[t]
        gae = delta + gamma * lam * nd * gae
        adv[t] = gae
    return adv, adv + val


def kl_adaptive(lr: float, kl: float, thr=0.008, factor=1.5, lr_min=1e-6, lr_max=1e-2) -> float:
    """skrl KLAdaptiveRL.step (kl_factor 2)."""
    if kl > thr * 2.0:
        return max(lr / factor, lr_min)
    if kl < thr / 2.0:
        return min(lr * factor, lr_max)
    return lr


class TorchLiftPPO:
    """The spec: skrl 1.1.0 PPO's update (PPO._update) on the lift networks with torch autograd and torch.optim.Adam."""

    def __init__(self, policy: LiftMLP, value: LiftMLP, lr: float = 1e-4, epochs: int = 8, minibatches: int = 24,
                 kl_early_stop: float = 0.008, max_grad_norm: float = 1.0, device="cuda"):
        self.policy, self.value = policy.to(device), value.to(device)
        self.device = torch.device(device)
        self.epochs, self.minibatches = int(epochs), int(minibatches)
        self.kl_early_stop, self.max_grad_norm = kl_early_stop, max_grad_norm
        self.opt = torch.optim.Adam(list(self.policy.parameters()) + list(self.value.parameters()), lr=lr)
        self.state_preprocessor = RunningStandardScaler(OBS_DIM, device=device)
        self.value_preprocessor = RunningStandardScaler(1, device=device)
        self.stopped_epochs = 0

    @property
    def lr(self) -> float:
        return self.opt.param_groups[0]["lr"]

    def update(self, obs, act, logp, val, ret, adv, perms=None):
        """PPO._update on flat (B, ...) buffers: raw states, standardised values / returns, normalised advantages.  The state
        scaler trains on every minibatch of the first epoch (``train=not epoch``); an epoch stops at the first minibatch whose
        KL exceeds kl_early_stop, before its optimiser step; KLAdaptiveRL after each epoch on the mean of the recorded KLs."""
        params = list(self.policy.parameters()) + list(self.value.parameters())
        B = obs.shape[0]
        kls_out = []
        for epoch in range(self.epochs):
            perm = perms[epoch] if perms is not None else torch.randperm(B, device=self.device)
            kls = []
            for mb in perm.chunk(self.minibatches):
                s = self.state_preprocessor(obs[mb], train=not epoch)
                loss, kl, _, _ = lift_ppo_loss(self.policy, self.value, s, act[mb], logp[mb], val[mb], ret[mb], adv[mb])
                kls.append(kl)
                if self.kl_early_stop and kl > self.kl_early_stop:
                    self.stopped_epochs += 1
                    break
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                nn.utils.clip_grad_norm_(params, self.max_grad_norm)
                self.opt.step()
            kl_mean = torch.stack(kls).mean().item()
            kls_out.append(kl_mean)
            lr = kl_adaptive(self.lr, kl_mean)
            for g in self.opt.param_groups:
                g["lr"] = lr
        return kls_out, self.lr

    def state_dict(self) -> dict:
        return {"policy": self.policy.state_dict(), "value": self.value.state_dict(),
                "state_preprocessor": self.state_preprocessor.state_dict(), "value_preprocessor": self.value_preprocessor.state_dict()}


# ---------------------------------------------------------------------------------------------------------------- HIP path
def _layers(sd: Mapping[str, torch.Tensor]):
    ws, bs, (n,) = _fused.host_layers(sd, (LIFT_KEY,))
    if n == 0:
        raise ValueError("state_dict has no net.<i>.weight entries")
    return ws, bs


def lift_desc(shapes) -> "_lib.PolicyDesc":
    """Descriptor of a lift-layout network (rover_lift_policy_desc for the skrl_ppo_cfg.yaml shapes)."""
    return make_desc(shapes, 0, "none", OBS_DIM, OBS_DIM, 0.01, hidden_act="elu")


def pack(sd: Mapping[str, torch.Tensor]):
    """(descriptor, packed host array) of a lift state_dict (``net.<2i>.*`` keys)."""
    ws, bs = _layers(sd)
    desc = lift_desc([w.shape for w in ws])
    return desc, _fused.pack_layers(desc, ws, bs)


def unpack(desc: "_lib.PolicyDesc", packed) -> dict:
    """Packed buffer (one replica) -> ``net.<2i>.*`` state_dict entries (rover_policy_unpack), float32 CPU tensors."""
    sd = {}
    for i, (w, b) in enumerate(zip(*_fused.unpack_layers(desc, packed))):
        sd[LIFT_KEY.format(2 * i, "weight")], sd[LIFT_KEY.format(2 * i, "bias")] = w, b
    return sd


def lift_net(sd: Mapping[str, torch.Tensor], **kw) -> RoverNet:
    """Inference network (``RoverNet``, one HIP launch) of a lift state_dict: ELU hidden layers, no final activation."""
    ws, bs = _layers(sd)
    return RoverNet(ws, bs, n_enc=0, final_act="none", obs_dim=OBS_DIM, prop_dim=OBS_DIM, hidden_act="elu", **kw)


def _scaler_block(width: int, device) -> torch.Tensor:
    blk = torch.zeros(2 * width + 1, dtype=torch.float64, device=device)   # mean 0, var 1, count 1
    blk[width:] = 1.0
    return blk


def _scaler_sd(blk: torch.Tensor, width: int) -> dict:
    b = blk.cpu()
    return {"running_mean": b[:width].clone(), "running_variance": b[width:2 * width].clone(), "current_count": b[2 * width].clone()}


class FusedLiftPPO(_fused.FusedActorCritic):
    """Lift PPO trainer state on the GPU: parameters, Adam moments, both scalers, learning rate, step count and the epoch's
    early-stop word all in device memory.  ``.actor`` / ``.critic`` alias the trainer's parameters (replicas refreshed by every
    optimiser step) and read STANDARDISED states (``standardize``).  ``update`` synchronises with the host once, at its end."""

    OBS_DIM, ACT_DIM = OBS_DIM, ACT_DIM
    _STATE, _WORKSPACE, _PARAM_FLOATS = _lib.LiftPpoState, "rover_lift_ppo_workspace_bytes", "rover_lift_ppo_param_floats"
    _RUNS = "the lift networks only (rover_lift_train.h)"
    _unpack = staticmethod(unpack)

    def __init__(self, policy_sd: Mapping[str, torch.Tensor], value_sd: Mapping[str, torch.Tensor], lr: float = 1e-4,
                 epochs: int = 8, minibatches: int = 24, device="cuda", n_copies: int = 4, **hparams):
        super().__init__(default_hparams, hparams, device, n_copies)
        self.epochs, self.minibatches = int(epochs), int(minibatches)
        self._networks(pack(policy_sd), pack(value_sd), policy_sd[LOG_STD_KEY])
        self.state = torch.zeros(C.sizeof(_lib.LiftPpoState) // 8, dtype=torch.float64, device=self.device)
        self.state[0] = float(lr)
        self.state_scaler = _scaler_block(OBS_DIM, self.device)
        self.value_scaler = _scaler_block(1, self.device)
        self._ensure_ws(1)

    @classmethod
    def from_checkpoint(cls, ck, **kw) -> "FusedLiftPPO":
        """skrl-style checkpoint ``{"policy", "value"[, "state_preprocessor", "value_preprocessor"]}`` (a path or the dict)."""
        ck = _fused.load_checkpoint(ck)
        t = super().from_checkpoint(ck, **kw)
        for key, blk, w in (("state_preprocessor", t.state_scaler, OBS_DIM), ("value_preprocessor", t.value_scaler, 1)):
            if key in ck:
                sd = ck[key]
                blk[:w] = torch.as_tensor(sd["running_mean"], dtype=torch.float64).reshape(-1).to(blk.device)
                blk[w:2 * w] = torch.as_tensor(sd["running_variance"], dtype=torch.float64).reshape(-1).to(blk.device)
                blk[2 * w] = float(torch.as_tensor(sd["current_count"]))
        return t

    # ---- views
    @property
    def lr(self) -> float:
        return float(self.state[0].item())

    def _word(self, i: int) -> int:
        return int(self.state.view(torch.int32)[i].item())

    @property
    def steps(self) -> int:
        return self._word(2)

    @property
    def stopped_epochs(self) -> int:
        return self._word(10)

    def state_dict(self) -> dict:
        """skrl-style checkpoint: ``policy`` / ``value`` state_dicts (``net.<2i>.*``, ``log_std_parameter``) and both scalers."""
        return {**super().state_dict(), "state_preprocessor": _scaler_sd(self.state_scaler, OBS_DIM),
                "value_preprocessor": _scaler_sd(self.value_scaler, 1)}

    # ---- kernels
    def standardize(self, x: torch.Tensor, which: str = "state", train: bool = False, inverse: bool = False,
                    out: torch.Tensor | None = None) -> torch.Tensor:
        """The state (36-wide) or value (1-wide) RunningStandardScaler on the device (rover_lift_ppo_standardize)."""
        blk, w = (self.state_scaler, OBS_DIM) if which == "state" else (self.value_scaler, 1)
        shape = x.shape
        x = x.reshape(-1, w)
        self._check(x, "x")
        out = torch.empty_like(x) if out is None else out
        _lib.check(self._lib.rover_lift_ppo_standardize(C.byref(self.hp), blk.data_ptr(), w, x.data_ptr(), int(x.shape[0]), int(train),
                                                        int(inverse), out.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                                        self._stream()), "rover_lift_ppo_standardize")
        return out.reshape(shape)

    def minibatch(self, obs, act, logp, val, ret, adv, idx, train_scaler=False, stats=None, mean_out=None, value_out=None):
        """Gradient of one minibatch into ``self.grad`` (nothing while the epoch's stop word is set); ``stats`` (4 floats)."""
        self._check(idx, "idx", torch.int64)
        n = int(idx.numel())
        self._ensure_ws(max(n, 1))
        if stats is None:
            stats = torch.zeros(4, device=self.device)
        _lib.check(self._lib.rover_lift_ppo_minibatch(C.byref(self.desc_p), C.byref(self.desc_v), C.byref(self.hp),
                                                      self.params.data_ptr(), self.state_scaler.data_ptr(), obs.data_ptr(),
                                                      act.data_ptr(), logp.data_ptr(), val.data_ptr(), ret.data_ptr(), adv.data_ptr(),
                                                      idx.data_ptr(), n, int(bool(train_scaler)), self.state.data_ptr(),
                                                      self.ws.data_ptr(), self.ws.numel(), self.grad.data_ptr(), stats.data_ptr(),
                                                      ptr(mean_out), ptr(value_out), self._stream()), "rover_lift_ppo_minibatch")
        return stats

    def apply(self):
        """clip_grad_norm_ + Adam on ``self.grad`` and the replica refresh (nothing while the stop word is set)."""
        _lib.check(self._lib.rover_lift_ppo_apply(C.byref(self.desc_p), C.byref(self.desc_v), C.byref(self.hp), self.params.data_ptr(),
                                                  self.grad.data_ptr(), self.adam_m.data_ptr(), self.adam_v.data_ptr(),
                                                  self.state.data_ptr(), self.rep_p.data_ptr(), self.rep_v.data_ptr(), self.n_copies,
                                                  self.ws.data_ptr(), self.ws.numel(), self._stream()), "rover_lift_ppo_apply")

    def kl_schedule(self, stats: torch.Tensor, kl_out: torch.Tensor | None = None):
        """KLAdaptiveRL from the epoch's recorded KLs ((n_minibatches, 4) stats), then the stop word cleared."""
        self._check(stats, "stats")
        _lib.check(self._lib.rover_lift_ppo_kl_schedule(C.byref(self.hp), stats.data_ptr(), int(stats.shape[0]), self.state.data_ptr(),
                                                        None if kl_out is None else kl_out.data_ptr(), self._stream()),
                   "rover_lift_ppo_kl_schedule")

    def update(self, obs, act, logp, val, ret, adv, perms=None, epochs: int | None = None, minibatches: int | None = None):
        """TorchLiftPPO.update on the device: raw states, standardised values / returns, normalised advantages, flat (B, ...)
        or (T, n_envs, ...).  Returns (epoch KL means, learning rate)."""
        epochs = self.epochs if epochs is None else int(epochs)
        mbs = self.minibatches if minibatches is None else int(minibatches)
        obs, act, logp, val, ret, adv, B = self._flat_rollout(obs, act, logp=logp, val=val, ret=ret, adv=adv)
        stats = torch.zeros(epochs, mbs, 4, device=self.device)
        kls = torch.empty(epochs, device=self.device)
        for e in range(epochs):
            for j, mb in enumerate(self._minibatches(perms, e, B, mbs)):
                self.minibatch(obs, act, logp, val, ret, adv, mb.contiguous(), train_scaler=(e == 0), stats=stats[e, j])
                self.apply()
            self.kl_schedule(stats[e], kls[e:e + 1])
        return kls.cpu().tolist(), self.lr
