"""Shared helpers of the SAC tests (test_sac.py, test_gpu_sac_update.py): the example's Gaussian actor, two Q(s, a) critics,
float64 / float32 copies, a fused trainer with both specs, and seeds picked on the float64 spec so that no clamp or min decision
of a run lies within a margin of its discontinuity.  td3_helpers' memory fill, error rule and workspace poison are reused."""
import copy

import torch

from ppo_reference import load_example
from td3_helpers import check, copies, err, fill, poison_ws  # noqa: F401  (re-exported for the SAC tests)


def nets(seed=0, device="cpu", bias=None, log_std=None):
    """(policy, critic_1, critic_2): Net(2, True) and two td3.Critic, float32.  ``bias`` sets the actor's output bias (pushes the
    mean towards the action bounds), ``log_std`` the log_std_parameter."""
    from isaac_rover_orbit_amd.td3 import Critic
    ex = load_example()
    torch.manual_seed(seed)
    pol, c1, c2 = ex.Net(2, True), Critic(), Critic()
    with torch.no_grad():
        if bias is not None:
            pol.mlp[6].bias.copy_(torch.tensor(bias))
        if log_std is not None:
            pol.log_std_parameter.copy_(torch.tensor(log_std))
    return pol.to(device), c1.to(device), c2.to(device)


def specs_of(mods, **hp):
    """{float64: TorchSAC, float32: TorchSAC} on copies of the modules."""
    from isaac_rover_orbit_amd.sac import TorchSAC
    return {dt: TorchSAC(*copies(mods, dt), **hp) for dt in (torch.float64, torch.float32)}


def trainers(mods, **fused_hp):
    """(FusedSAC, specs) with the same networks; ``learn_entropy`` is the one hyper-parameter both take by that name."""
    from isaac_rover_orbit_amd.sac import FusedSAC
    torch_hp = {k: v for k, v in fused_hp.items() if k == "learn_entropy"}
    fused = FusedSAC(*(m.state_dict() for m in mods), **fused_hp)
    return fused, specs_of(mods, **torch_hp)


def sample(mem, idx, dt):
    s, a, r, s2, t = mem.gather(idx)
    return s.to(dt), a.to(dt), r.to(dt), s2.to(dt), t


def grads(module):
    return {k: p.grad.detach().clone() for k, p in module.named_parameters()}


def params(module):
    return {k: p.detach().clone() for k, p in module.named_parameters()}


def draws(n, seed, device="cpu", scale=1.0):
    """eps (n, 4) float32: columns 0:2 for s', columns 2:4 for s."""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(n, 4, device=device, generator=g) * scale


def _margin(spec, st, e, qa, qb):
    from isaac_rover_orbit_amd.sac import LOG_STD_MAX, LOG_STD_MIN
    with torch.no_grad():
        sigma = spec.policy.log_std_parameter.clamp(LOG_STD_MIN, LOG_STD_MAX).exp()
        x = spec.policy(st) + sigma * e.to(spec.dtype)
        u = x.clamp(-1.0, 1.0)
        return min(float((x.abs() - 1.0).abs().min()), float((qa(st, u) - qb(st, u)).abs().min()))


def update_with_margin(spec, mem, idx, eps):
    """``spec.update(mem, idx, eps)`` in its pieces; returns the smallest | |x| - 1 | and | q1 - q2 | over the rows, each read where
    the update decides it: the target pair on (s', u') before the critic step, the critics on (s, u) after it."""
    s, a, r, s2, t = sample(mem, idx, spec.dtype)
    m = _margin(spec, s2, eps[:, 0:2], spec.target_critic_1, spec.target_critic_2)
    spec.critic_step(s, a, r, s2, t, eps[:, 0:2])
    m = min(m, _margin(spec, s, eps[:, 2:4], spec.critic_1, spec.critic_2))
    spec.policy_step(s, eps[:, 2:4])
    spec.polyak()
    return m


def clone_modules(mods):
    return [copy.deepcopy(m) for m in mods]
