"""Float64 restatement of the PPO minibatch loss of examples/04_train_ppo.py (``ppo_loss``), written independently with
torch.nn.functional on a flat dict of parameters, for checking the fused update's gradients.  Test infrastructure only."""
import importlib.util
import os

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENC = ["dense_encoder.encoder_layers.0", "dense_encoder.encoder_layers.2"]
MLP = ["mlp.0", "mlp.2", "mlp.4", "mlp.6"]


def load_example():
    """examples/04_train_ppo.py as a module (its ``Net`` and ``ppo_loss`` are the specification)."""
    spec = importlib.util.spec_from_file_location("train_ppo_example", os.path.join(ROOT, "examples", "04_train_ppo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def net_forward(sd, s, final_tanh):
    e = s[:, 3:-1]
    for k in ENC:
        e = F.leaky_relu(F.linear(e, sd[k + ".weight"], sd[k + ".bias"]), 0.01)
    x = torch.cat([s[:, 0:4], e], 1)
    for i, k in enumerate(MLP):
        x = F.linear(x, sd[k + ".weight"], sd[k + ".bias"])
        if i < len(MLP) - 1:
            x = F.leaky_relu(x, 0.01)
    return torch.tanh(x) if final_tanh else x


def loss_and_grads(policy_sd, value_sd, o, a, old_lp, old_v, ret, adv, clip=0.2, vclip=0.2, dtype=torch.float64):
    """(loss, kl, grads) with grads = {"policy": {key: grad}, "value": {key: grad}} in ``dtype`` on the inputs' device."""
    P = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in policy_sd.items()}
    V = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in value_sd.items()}
    o, a, old_lp, old_v, ret, adv = (x.to(dtype) for x in (o, a, old_lp, old_v, ret, adv))
    mean = net_forward(P, o, True)
    ls = torch.clamp(P["log_std_parameter"], -20.0, 2.0)
    z = (a - mean) / torch.exp(ls)
    lp = torch.sum(-0.5 * z * z - ls - 0.9189385332, dim=1)
    log_r = lp - old_lp
    r = torch.exp(log_r)
    kl = torch.mean((r - 1) - log_r).detach()
    policy_loss = -torch.mean(torch.minimum(r * adv, torch.clamp(r, 1 - clip, 1 + clip) * adv))
    v = net_forward(V, o, False)[:, 0]
    v = old_v + torch.clamp(v - old_v, -vclip, vclip)
    value_loss = torch.mean((ret - v) ** 2)
    loss = policy_loss + value_loss
    loss.backward()
    return loss.detach(), kl, {"policy": {k: t.grad for k, t in P.items()}, "value": {k: t.grad for k, t in V.items()}}
