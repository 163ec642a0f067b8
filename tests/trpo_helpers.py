"""Shared helpers of the fused TRPO tests (test_gpu_trpo_update.py, test_gpu_trpo_edges.py): the example's networks, synthetic
rollouts, float64 / float32 copies of a network and the "fused error <= 4x torch fp32 error against float64, plus a floor" check."""
import torch

from ppo_reference import load_example

DEV = "cuda"


def _nets(seed=0, log_std=(-0.4, 0.3)):
    ex = load_example()
    torch.manual_seed(seed)
    pol, val = ex.Net(2, True), ex.Net(1, False)
    with torch.no_grad():
        pol.log_std_parameter.copy_(torch.tensor(log_std))
    return pol.to(DEV), val.to(DEV)


def _rollout(pol, B, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    obs = torch.randn(B, 965, device=DEV, generator=g) * 0.5
    with torch.no_grad():
        mean = torch.cat([pol(obs[i:i + 8192]) for i in range(0, B, 8192)])
        ls = pol.log_std_parameter.clamp(-20.0, 2.0)
        act = mean + ls.exp() * torch.randn(B, 2, device=DEV, generator=g)
        lp = (-0.5 * ((act - mean) / ls.exp()) ** 2 - ls - 0.9189385332).sum(1)
    logp = (lp + 0.05 * torch.randn(B, device=DEV, generator=g)).contiguous()
    adv = torch.randn(B, device=DEV, generator=g)
    if B > 1:                                                   # one row has no standard deviation
        adv = ((adv - adv.mean()) / (adv.std() + 1e-8)).contiguous()
    ret = torch.randn(B, device=DEV, generator=g)
    return obs, act.contiguous(), logp, ret, adv


def _copy(net, dtype):
    import copy
    return copy.deepcopy(net).to(dtype)


def _flat_to_sd(net, flat):
    out, i = {}, 0
    for k, p in net.named_parameters():
        out[k] = flat[i:i + p.numel()].view_as(p)
        i += p.numel()
    return out


def _err(a, ref):
    return float((a.double().cpu() - ref.double().cpu()).norm())


def _check(fused_sd, sd64, sd32, factor=4.0, floor=1e-5):
    for k, ref in sd64.items():
        e_f, e_t = _err(fused_sd[k], ref), _err(sd32[k], ref)
        assert e_f <= factor * e_t + floor * float(ref.double().norm()) + 1e-30, (k, e_f, e_t, float(ref.norm()))


def _trainer(pol, val, **kw):
    from isaac_rover_orbit_amd.trpo import FusedTRPO
    return FusedTRPO(pol.state_dict(), val.state_dict(), **kw)


def _spec_step(pol, val, obs, act, logp, adv, dtype, **hp):
    from isaac_rover_orbit_amd.trpo import TorchTRPO
    p, v = _copy(pol, dtype), _copy(val, dtype)
    st = TorchTRPO(p, v, **hp).policy_step(obs.to(dtype), act.to(dtype), logp.to(dtype), adv.to(dtype))
    return p, st
