"""Float64 restatement of the lift PPO minibatch loss (isaac_rover_orbit_amd.lift_ppo.lift_ppo_loss) and of skrl's
RunningStandardScaler, written independently with torch.nn.functional / numpy on flat parameter dicts, for checking the fused
update.  Test infrastructure only."""
import numpy as np
import torch
import torch.nn.functional as F

LAYERS = ["net.0", "net.2", "net.4", "net.6"]


def net_forward(sd, s):
    x = s
    for i, k in enumerate(LAYERS):
        x = F.linear(x, sd[k + ".weight"], sd[k + ".bias"])
        if i < len(LAYERS) - 1:
            x = F.elu(x)
    return x


def loss_terms_and_grads(policy_sd, value_sd, s, a, old_lp, old_v, ret, adv, clip=0.2, vclip=0.2, vscale=2.0, ls_min=-20.0,
                         ls_max=2.0, dtype=torch.float64):
    """(loss, kl, policy loss, scaled value loss, grads) on STANDARDISED states s; grads = {"policy": {key: grad},
    "value": {key: grad}} in ``dtype``.  torch.clamp passes the gradient on the closed interval [ls_min, ls_max]."""
    P = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in policy_sd.items()}
    V = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in value_sd.items()}
    s, a, old_lp, old_v, ret, adv = (x.to(dtype) for x in (s, a, old_lp, old_v, ret, adv))
    mean = net_forward(P, s)
    ls = torch.clamp(P["log_std_parameter"], ls_min, ls_max)
    z = (a - mean) / torch.exp(ls)
    lp = torch.sum(-0.5 * z * z - ls - 0.9189385332, dim=1)
    log_r = lp - old_lp
    r = torch.exp(log_r)
    kl = torch.mean((r - 1) - log_r).detach()
    policy_loss = -torch.mean(torch.minimum(r * adv, torch.clamp(r, 1 - clip, 1 + clip) * adv))
    v = net_forward(V, s)[:, 0]
    v = old_v + torch.clamp(v - old_v, -vclip, vclip)
    value_loss = vscale * F.mse_loss(v, ret)
    loss = policy_loss + value_loss
    loss.backward()
    grads = {"policy": {k: t.grad for k, t in P.items()}, "value": {k: t.grad for k, t in V.items()}}
    return loss.detach(), kl, policy_loss.detach(), value_loss.detach(), grads


def loss_and_grads(policy_sd, value_sd, s, a, old_lp, old_v, ret, adv, clip=0.2, vclip=0.2, vscale=2.0, ls_min=-20.0, ls_max=2.0,
                   dtype=torch.float64):
    """(loss, kl, grads) of loss_terms_and_grads."""
    loss, kl, _, _, grads = loss_terms_and_grads(policy_sd, value_sd, s, a, old_lp, old_v, ret, adv, clip=clip, vclip=vclip,
                                                 vscale=vscale, ls_min=ls_min, ls_max=ls_max, dtype=dtype)
    return loss, kl, grads


def clip_and_adam(params64, grads64, m, v, step, lr, max_norm, beta1, beta2, eps, dtype=torch.float64):
    """torch.nn.utils.clip_grad_norm_(max_norm) followed by one torch.optim.Adam step (the ``step``-th, 1-based; no weight
    decay, no amsgrad), written out in ``dtype`` over flat lists of tensors in torch's order of operations.  Returns
    (params, m, v, clipped grads, norm, clip coefficient): new lists in ``dtype``, the last two as Python floats."""
    params = [p.detach().to(dtype).clone() for p in params64]
    grads = [g.detach().to(dtype).clone() for g in grads64]
    m = [t.detach().to(dtype).clone() for t in m]
    v = [t.detach().to(dtype).clone() for t in v]
    # clip_grad_norm_: the 2-norm of the per-tensor 2-norms, coefficient max_norm / (norm + 1e-6) clamped to 1
    norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    for g in grads:
        g.mul_(coef)
    # torch.optim.Adam (_single_tensor_adam)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    step_size = lr / bc1
    bc2_sqrt = bc2 ** 0.5
    for p, g, ea, es in zip(params, grads, m, v):
        ea.lerp_(g, 1 - beta1)
        es.mul_(beta2).addcmul_(g, g, value=1 - beta2)
        denom = (es.sqrt() / bc2_sqrt).add_(eps)
        p.addcdiv_(ea, denom, value=-step_size)
    return params, m, v, grads, float(norm), float(coef)


class NumpyScaler:
    """skrl RunningStandardScaler in float64 numpy: parallel-variance merge of the batch mean and unbiased variance."""

    def __init__(self, width, eps=1e-8, clip=5.0):
        self.mean, self.var, self.count = np.zeros(width), np.ones(width), 1.0
        self.eps, self.clip = eps, clip

    def train(self, x):
        x = np.asarray(x, np.float64)
        bm, bv, bc = x.mean(0), x.var(0, ddof=1), x.shape[0]
        delta = bm - self.mean
        tot = self.count + bc
        m2 = self.var * self.count + bv * bc + delta ** 2 * self.count * bc / tot
        self.mean = self.mean + delta * bc / tot
        self.var = m2 / tot
        self.count = tot

    def forward(self, x):
        return np.clip((x - self.mean) / (np.sqrt(self.var) + self.eps), -self.clip, self.clip)

    def inverse(self, x):
        return np.sqrt(self.var) * np.clip(x, -self.clip, self.clip) + self.mean
