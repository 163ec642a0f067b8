"""TRPO for the rover's actor and critic: the torch spec (skrl 1.x ``TRPO._update``) and the fused HIP update on the MI355X
(C ABI: ``include/rover_trpo.h``).

``TorchTRPO`` restates skrl's TRPO with the reference's ``rover_trpo.yaml`` on the networks of ``examples/04_train_ppo.py``
(``Net``): surrogate gradient, conjugate gradient on double-backward Fisher-vector products, the backtracking line search with
skrl's cumulative expected improvement, then the value regression with ``clip_grad_norm_`` and Adam.  skrl is not a dependency;
each function names the skrl function it follows.  Where skrl's behaviour is stated from memory it is a hyper-parameter.

``FusedTRPO`` runs the same update as HIP kernels on one flat device vector in ``FusedPPO``'s layout (policy packed, value
packed, ``log_std`` + 2 padding).  ``.actor`` / ``.critic`` alias the trainer's parameters.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping

import numpy as np
import torch
import torch.nn as nn

from . import _fused, _lib
from ._fused import ptr
from .ppo import LOG_STD_KEY, pack, unpack

# skrl TRPO_DEFAULT_CONFIG with rover_trpo.yaml.  The yaml's learning_rate (1e-4) is not a TRPO key: skrl's TRPO reads
# value_learning_rate (1e-3) for the value optimiser and has no policy optimiser.  Both values stay reachable here.
HPARAMS = dict(rollouts=60, learning_epochs=4, mini_batches=60, discount_factor=0.99, lambda_=0.95, value_loss_scale=1.0,
               grad_norm_clip=0.5, damping=0.1, max_kl_divergence=0.01, conjugate_gradient_steps=10, cg_residual_tolerance=1e-10,
               max_backtrack_steps=10, accept_ratio=0.5, step_fraction=1.0, value_learning_rate=1e-3, learning_rate=1e-4,
               log_std_min=-20.0, log_std_max=2.0)


# ---------------------------------------------------------------------------------------------------------------- torch spec
def _log_std(policy) -> torch.Tensor:
    """GaussianMixin.act: the clamped log_std that ``get_log_std`` hands back (gradient passes inside the clamp)."""
    return policy.log_std_parameter.clamp(HPARAMS["log_std_min"], HPARAMS["log_std_max"])


def log_prob(policy, states, actions):
    """GaussianMixin.act: Normal(mean, exp(log_std)).log_prob(actions).sum(-1), written out as examples/04_train_ppo.py does."""
    mean = policy(states)
    ls = _log_std(policy)
    return (-0.5 * ((actions - mean) / ls.exp()) ** 2 - ls - 0.9189385332).sum(1)


def surrogate_loss(policy, states, actions, log_prob_old, advantages):
    """skrl TRPO._update.surrogate_loss: (advantages * exp(new_log_prob - log_prob.detach())).mean()."""
    return (advantages * torch.exp(log_prob(policy, states, actions) - log_prob_old.detach())).mean()


def kl_divergence(policy_1, policy_2, states):
    """skrl TRPO._update.kl_divergence: mean over rows of sum_i KL(N(mu_1, s_1) || N(mu_2, s_2)); policy_1 detached."""
    mu_1, logstd_1 = policy_1(states).detach(), _log_std(policy_1).detach()
    mu_2, logstd_2 = policy_2(states), _log_std(policy_2)
    kl = logstd_1 - logstd_2 + 0.5 * (torch.square(logstd_1.exp()) + torch.square(mu_1 - mu_2)) / torch.square(logstd_2.exp()) - 0.5
    return torch.sum(kl, dim=-1).mean()


def fisher_vector_product(policy, states, vector, damping=0.1):
    """skrl TRPO._update.fisher_vector_product: double-backward of kl_divergence(policy, policy) plus damping * vector."""
    kl = kl_divergence(policy, policy, states)
    kl_gradient = torch.autograd.grad(kl, list(policy.parameters()), create_graph=True)
    flat_kl_gradient = torch.cat([gradient.view(-1) for gradient in kl_gradient])
    hessian_vector_gradient = torch.autograd.grad((flat_kl_gradient * vector).sum(), list(policy.parameters()))
    flat_hessian_vector_gradient = torch.cat([gradient.contiguous().view(-1) for gradient in hessian_vector_gradient])
    return flat_hessian_vector_gradient + damping * vector


def gauss_newton_fvp(policy, states, vector, damping=0.1):
    """The closed form the kernels implement: (1/B) J^T diag(sigma^-2) J v_w on the network, 2 c_i v_s,i on log_std, no cross
    terms, plus damping v -- one forward-mode product (torch.func.jvp) and one reverse product (torch.func.vjp)."""
    from torch.func import functional_call, jvp, vjp
    names = [n for n, _ in policy.named_parameters()]
    params = dict(policy.named_parameters())
    net = [n for n in names if n != "log_std_parameter"]
    chunks = dict(zip(names, torch.split(vector, [p.numel() for p in params.values()])))
    tang = {n: chunks[n].view_as(params[n]) for n in net}
    prim = {n: params[n].detach() for n in net}
    fixed = {"log_std_parameter": params["log_std_parameter"].detach()}
    f = lambda p: functional_call(policy, {**p, **fixed}, (states,))  # noqa: E731
    _, jv = jvp(f, (prim,), (tang,))
    ls = fixed["log_std_parameter"]
    sig2 = torch.exp(2 * ls.clamp(HPARAMS["log_std_min"], HPARAMS["log_std_max"]))
    _, pull = vjp(f, prim)
    (gw,) = pull(jv / sig2 / states.shape[0])
    c = ((ls >= HPARAMS["log_std_min"]) & (ls <= HPARAMS["log_std_max"])).to(vector.dtype)
    out = [2 * c * chunks["log_std_parameter"] if n == "log_std_parameter" else gw[n].reshape(-1) for n in names]
    return torch.cat(out) + damping * vector


def conjugate_gradient(fvp, b, num_iterations=10, residual_tolerance=1e-10, trace: list | None = None):
    """skrl TRPO._update.conjugate_gradient; returns (x, iterations run, final r.r).  ``trace`` (a list) receives r.r after
    each iteration."""
    x = torch.zeros_like(b)
    r = b.clone()
    p = b.clone()
    rr_old = torch.dot(r, r)
    rr_new, it = rr_old, 0
    for it in range(1, num_iterations + 1):
        hv = fvp(p)
        alpha = rr_old / torch.dot(p, hv)
        x += alpha * p
        r -= alpha * hv
        rr_new = torch.dot(r, r)
        if trace is not None:
            trace.append(float(rr_new))
        if rr_new < residual_tolerance:
            break
        p = r + rr_new / rr_old * p
        rr_old = rr_new
    return x, it, float(rr_new)


def line_search(params_old, full_step, expected_improvement, evaluate, loss_old, max_kl, accept_ratio, step_fraction=1.0,
                max_backtrack_steps=10):
    """skrl TRPO._update's backtracking loop.  evaluate(theta) -> (kl, surrogate).  expected_improvement is multiplied by each
    alpha in turn (skrl's ``expected_improvement *= alpha``: a cumulative product).  Returns (accepted trial or -1, theta, kl,
    surrogate); with no trial accepted theta is ``params_old`` itself (restored bit for bit)."""
    kl = loss = float("nan")
    for i, alpha in enumerate([step_fraction * 0.5 ** i for i in range(max_backtrack_steps)]):
        new_params = params_old + alpha * full_step
        expected_improvement = expected_improvement * alpha
        kl, loss = evaluate(new_params)
        if kl < max_kl and (loss - loss_old) / expected_improvement > accept_ratio:
            return i, new_params, kl, loss
    return -1, params_old, kl, loss


class TorchTRPO:
    """skrl TRPO._update in torch autograd on ``Net(2, True)`` / ``Net(1, False)`` of examples/04_train_ppo.py."""

    def __init__(self, policy: nn.Module, value: nn.Module, **hparams):
        self.policy, self.value = policy, value
        self.hp = dict(HPARAMS)
        for k, v in hparams.items():
            if k not in self.hp:
                raise TypeError(f"unknown hyper-parameter {k!r}")
            self.hp[k] = v
        self.value_optimizer = torch.optim.Adam(self.value.parameters(), lr=self.hp["value_learning_rate"])

    def _vector(self):
        return nn.utils.parameters_to_vector(self.policy.parameters())

    def policy_step(self, obs, act, logp, adv) -> dict:
        """Steps 1-5 over all rows (skrl samples the policy tensors with mini_batches=1)."""
        hp, policy = self.hp, self.policy
        policy_loss = surrogate_loss(policy, obs, act, logp, adv)
        grads = torch.autograd.grad(policy_loss, list(policy.parameters()))
        g = torch.cat([gr.view(-1) for gr in grads])
        fvp = lambda v: fisher_vector_product(policy, obs, v, hp["damping"])  # noqa: E731
        x, iters, rr = conjugate_gradient(fvp, g.data, hp["conjugate_gradient_steps"], hp["cg_residual_tolerance"])
        xhx = (x * fvp(x)).sum(0, keepdim=True)
        step = torch.sqrt(2 * hp["max_kl_divergence"] / xhx)[0]
        full = step * x
        expected = (g * full).sum(0, keepdim=True)
        backup = [p.detach().clone() for p in policy.parameters()]
        with torch.no_grad():
            old_mean = policy(obs)
            old_ls = _log_std(policy)
            theta_old = self._vector()

            def evaluate(theta):
                nn.utils.vector_to_parameters(theta, policy.parameters())
                mu, ls = policy(obs), _log_std(policy)
                kl = (old_ls - ls + 0.5 * (torch.square(old_ls.exp()) + torch.square(old_mean - mu)) / torch.square(ls.exp()) - 0.5)
                return kl.sum(-1).mean(), surrogate_loss(policy, obs, act, logp, adv)

            acc, _, kl, loss = line_search(theta_old, full, expected, evaluate, policy_loss.detach(), hp["max_kl_divergence"],
                                           hp["accept_ratio"], hp["step_fraction"], hp["max_backtrack_steps"])
            if acc < 0:                                             # policy.update_parameters(backup_policy)
                for p, b in zip(policy.parameters(), backup):
                    p.copy_(b)
        return {"loss_old": float(policy_loss.detach()), "cg_iters": iters, "cg_rr": rr, "xhx": float(xhx), "step": float(step),
                "accepted": acc, "kl": float(kl), "grad": g.detach(), "direction": x.detach()}

    def value_pass(self, obs, ret, perms) -> float:
        """learning_epochs x mini_batches of value_loss_scale * mse, clip_grad_norm_(value), Adam; returns the mean loss."""
        hp, losses = self.hp, []
        for perm in perms:
            for mb in perm.chunk(hp["mini_batches"]):
                pred = self.value(obs[mb]).squeeze(1)
                value_loss = hp["value_loss_scale"] * torch.nn.functional.mse_loss(ret[mb], pred)
                self.value_optimizer.zero_grad()
                value_loss.backward()
                nn.utils.clip_grad_norm_(self.value.parameters(), hp["grad_norm_clip"])
                self.value_optimizer.step()
                losses.append(value_loss.detach())
        return float(torch.stack(losses).mean())

    def update(self, obs, act, logp, ret, adv, perms=None) -> dict:
        obs = obs.reshape(-1, obs.shape[-1])
        B = obs.shape[0]
        act, logp, ret, adv = act.reshape(B, -1), logp.reshape(B), ret.reshape(B), adv.reshape(B)
        st = self.policy_step(obs, act, logp, adv)
        st.pop("grad"); st.pop("direction")
        if perms is None:
            perms = [torch.randperm(B, device=obs.device) for _ in range(self.hp["learning_epochs"])]
        st["value_loss"] = self.value_pass(obs, ret, perms)
        return st


# ---------------------------------------------------------------------------------------------------------------- fused
def default_hparams() -> "_lib.TrpoHparams":
    return _fused.default_hparams(_lib.TrpoHparams, "rover_trpo_default_hparams")


STAT_KEYS = ("loss_old", "cg_iters", "cg_rr", "xhx", "step", "accepted", "kl", "value_loss")


class FusedTRPO(_fused.FusedActorCritic):
    """TRPO trainer state on the GPU: parameters, value Adam moments and the device state struct (rover_trpo_state).

    ``update`` synchronises with the host once, at its end, to return the statistics.  ``from_checkpoint`` takes a skrl checkpoint
    ``{"policy": state_dict, "value": state_dict, ...}`` (a path or the loaded dict).
    """

    _STATE, _WORKSPACE, _PARAM_FLOATS = _lib.TrpoState, "rover_trpo_workspace_bytes", "rover_trpo_param_floats"
    _RUNS = "the reference architecture only (rover_trpo.h)"
    _PAD = 2
    _unpack = staticmethod(unpack)

    def __init__(self, policy_sd: Mapping[str, torch.Tensor], value_sd: Mapping[str, torch.Tensor], epochs: int = 4,
                 minibatches: int = 60, device="cuda", n_copies: int = 4, **hparams):
        super().__init__(default_hparams, hparams, device, n_copies)
        self.epochs, self.minibatches = int(epochs), int(minibatches)
        self._networks(pack(policy_sd, "tanh"), pack(value_sd, "none"), policy_sd[LOG_STD_KEY])
        self.state = torch.zeros(C.sizeof(_lib.TrpoState) // 4, dtype=torch.int32, device=self.device)
        self._ws_shape = (0, 0)

    # ---- views
    def vector(self, policy_sd: Mapping[str, torch.Tensor]) -> torch.Tensor:
        """A policy-side device vector (this class's layout, value block and padding zero) from state_dict-shaped tensors."""
        _, pa = pack(policy_sd, "tanh")
        ls = torch.as_tensor(policy_sd[LOG_STD_KEY]).detach().float().cpu().reshape(-1).numpy()
        return torch.from_numpy(np.concatenate([pa, np.zeros(self.n_v, np.float32), ls, np.zeros(2, np.float32)])).to(self.device)

    def unvector(self, vec: torch.Tensor) -> dict:
        """The inverse of ``vector``: state_dict-shaped float32 CPU tensors of a policy-side vector."""
        v = vec.detach().cpu()
        sd = unpack(self.desc_p, v[:self.n_p])
        sd[LOG_STD_KEY] = v[self.n_p + self.n_v:self.n_p + self.n_v + 2].clone()
        return sd

    # ---- kernels
    def _ensure_ws(self, rows: int, mb: int = 1):
        """Grow the workspace to (rows, mb).  The old bytes are carried over (on the stream of the kernels): the policy region
        sits at a fixed offset and its layout depends on the caller's B only, so the theta_old cache ``fvp`` reads survives a
        growth by ``value_minibatch`` between ``policy_grad`` and ``fvp``."""
        rows, mb = max(rows, self._ws_shape[0]), max(mb, self._ws_shape[1])
        if (rows, mb) != self._ws_shape:
            need = int(self._ws_bytes(rows, mb))
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            ws[:self.ws.numel()].copy_(self.ws)
            self.ws = ws
            self._ws_shape = (rows, mb)

    def _rollout(self, obs, act, logp, adv):
        return self._flat_rollout(obs, act, logp=logp, adv=adv)

    def policy_grad(self, obs, act, logp, adv) -> torch.Tensor:
        """Step 1 at the current parameters: g into ``self.grad`` (value block zero); caches theta_old for ``fvp``."""
        obs, act, logp, adv, B = self._rollout(obs, act, logp, adv)
        self._ensure_ws(B)
        self._B = B
        _lib.check(self._lib.rover_trpo_policy_grad(C.byref(self.desc_p), C.byref(self.desc_v), C.byref(self.hp), self.params.data_ptr(),
                                                    obs.data_ptr(), act.data_ptr(), logp.data_ptr(), adv.data_ptr(), B, self.ws.data_ptr(),
                                                    self.ws.numel(), self.grad.data_ptr(), self.state.data_ptr(), self._stream()),
                   "rover_trpo_policy_grad")
        return self.grad

    def fvp(self, obs, v: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """F v + damping v at the theta_old of the last ``policy_grad`` (same obs)."""
        obs = obs.reshape(-1, obs.shape[-1])
        self._check(obs, "obs")
        self._check(v, "v")
        if obs.shape[0] != getattr(self, "_B", -1):
            raise ValueError("fvp needs policy_grad on the same rows first")
        out = torch.empty_like(self.params) if out is None else out
        _lib.check(self._lib.rover_trpo_fvp(C.byref(self.desc_p), C.byref(self.desc_v), C.byref(self.hp), self.params.data_ptr(),
                                            obs.data_ptr(), self._B, self.ws.data_ptr(), self.ws.numel(), v.data_ptr(), out.data_ptr(),
                                            self._stream()), "rover_trpo_fvp")
        return out

    def policy_step(self, obs, act, logp, adv, grad_out=None, dir_out=None):
        """Steps 1-5 (gradient, CG, step, line search or restore) on the device; replicas of ``.actor`` refreshed."""
        obs, act, logp, adv, B = self._rollout(obs, act, logp, adv)
        self._ensure_ws(B)
        self._B = B
        _lib.check(self._lib.rover_trpo_policy_step(C.byref(self.desc_p), C.byref(self.desc_v), C.byref(self.hp), self.params.data_ptr(),
                                                    obs.data_ptr(), act.data_ptr(), logp.data_ptr(), adv.data_ptr(), B, self.ws.data_ptr(),
                                                    self.ws.numel(), self.state.data_ptr(), self.rep_p.data_ptr(), self.n_copies,
                                                    ptr(grad_out), ptr(dir_out), self._stream()), "rover_trpo_policy_step")

    def value_minibatch(self, obs, ret, idx):
        """The value loss gradient of rows ``idx`` into the value block of ``self.grad``; the loss adds to the state."""
        obs = obs.reshape(-1, obs.shape[-1])
        ret = ret.reshape(-1)
        self._check(obs, "obs"); self._check(ret, "ret"); self._check(idx, "idx", torch.int64)
        rows, n = obs.shape[0], int(idx.numel())
        self._ensure_ws(rows, n)
        _lib.check(self._lib.rover_trpo_value_minibatch(C.byref(self.desc_p), C.byref(self.desc_v), C.byref(self.hp), self.params.data_ptr(),
                                                        obs.data_ptr(), ret.data_ptr(), idx.data_ptr(), n, self._ws_shape[0],
                                                        self.ws.data_ptr(), self.ws.numel(), self.grad.data_ptr(), self.state.data_ptr(),
                                                        self._stream()), "rover_trpo_value_minibatch")

    def value_apply(self):
        """clip_grad_norm_(value) + Adam on the value block, then the replicas ``.critic`` reads."""
        self._ensure_ws(1)
        _lib.check(self._lib.rover_trpo_value_apply(C.byref(self.desc_p), C.byref(self.desc_v), C.byref(self.hp), self.params.data_ptr(),
                                                    self.grad.data_ptr(), self.adam_m.data_ptr(), self.adam_v.data_ptr(),
                                                    self.state.data_ptr(), self.rep_v.data_ptr(), self.n_copies, self.ws.data_ptr(),
                                                    self.ws.numel(), self._stream()), "rover_trpo_value_apply")

    def update(self, obs, act, logp, ret, adv, perms=None) -> dict:
        """One TRPO update on flat (B, ...) or (T, n_envs, ...) buffers: the policy step, then ``epochs`` passes over
        ``torch.randperm(B).chunk(minibatches)`` (or the given ``perms[epoch]``) of the value regression.  Returns the
        statistics (``STAT_KEYS``) with one host synchronisation."""
        obs, act, logp, adv, B = self._rollout(obs, act, logp, adv)
        ret = ret.reshape(B)
        self._check(ret, "ret")
        self._ensure_ws(B, -(-B // self.minibatches))
        self.policy_step(obs, act, logp, adv)
        for e in range(self.epochs):
            for mb in self._minibatches(perms, e, B, self.minibatches):
                self.value_minibatch(obs, ret, mb.contiguous())
                self.value_apply()
        s = self.stats()
        return {"loss_old": s["loss_old"], "cg_iters": s["cg_iters"], "cg_rr": s["rr"], "xhx": s["xhx"], "step": s["step"],
                "accepted": s["accepted"], "kl": s["kl"], "value_loss": s["value_loss_sum"] / max(s["value_batches"], 1)}
