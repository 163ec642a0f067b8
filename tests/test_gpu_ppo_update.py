"""Fused PPO update on the MI355X (include/rover_train.h, isaac_rover_orbit_amd.ppo) against examples/04_train_ppo.py: the
training forward is bit-identical to RoverNet, gradients agree with float64 autograd as closely as torch fp32 does, clip + Adam
follow torch, GAE is bit-identical to the example's loop, one whole update tracks the example's torch update."""
import ctypes as C

import numpy as np
import pytest
import torch

from ppo_reference import load_example, loss_and_grads

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _nets(seed=0, log_std=(-0.4, 0.3)):
    ex = load_example()
    torch.manual_seed(seed)
    pol, val = ex.Net(2, True), ex.Net(1, False)
    with torch.no_grad():
        pol.log_std_parameter.copy_(torch.tensor(log_std))
    return ex, pol, val


def _rollout(pol, val, T, n, seed=1, lp_noise=0.3, v_noise=0.4):
    """Synthetic flat rollout buffers (T * n rows) whose ratios and value errors cross every clip branch."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    B = T * n
    obs = torch.randn(B, 965, device=DEV, generator=g) * 0.5
    with torch.no_grad():
        p, v = pol.to(DEV), val.to(DEV)
        mean = torch.cat([p(obs[i:i + 8192]) for i in range(0, B, 8192)])
        v0 = torch.cat([v(obs[i:i + 8192])[:, 0] for i in range(0, B, 8192)])
        ls = p.log_std_parameter.clamp(-20.0, 2.0)
        act = mean + ls.exp() * torch.randn(B, 2, device=DEV, generator=g)
        lp = (-0.5 * ((act - mean) / ls.exp()) ** 2 - ls - 0.9189385332).sum(1)
    logp = (lp + lp_noise * torch.randn(B, device=DEV, generator=g)).contiguous()
    oldv = (v0 + v_noise * torch.randn(B, device=DEV, generator=g)).contiguous()
    ret = (oldv + torch.randn(B, device=DEV, generator=g)).contiguous()
    adv = torch.randn(B, device=DEV, generator=g)
    return obs, act.contiguous(), logp, oldv, ret, adv


def _trainer(pol, val, **kw):
    from isaac_rover_orbit_amd.ppo import FusedPPO
    return FusedPPO(pol.state_dict(), val.state_dict(), **kw)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4096])
def test_training_forward_is_bit_identical_to_rovernet(n):
    from isaac_rover_orbit_amd.policy import RoverNet
    ex, pol, val = _nets(0)
    T, E = 60, 4096
    obs, act, logp, oldv, ret, adv = _rollout(pol, val, 2, E)
    big = torch.zeros(T * E, 965, device=DEV)                       # rows far apart in a 60 x 4096 buffer
    big[:2 * E] = obs
    big[-2 * E:] = obs
    g = torch.Generator(device=DEV).manual_seed(n)
    idx = torch.randint(0, T * E, (n,), device=DEV, generator=g)
    if n > 3:
        idx[1] = idx[0]                                             # a repeat
        idx[2] = T * E - 1                                          # the very last row
    big[idx] = torch.randn(n, 965, device=DEV, generator=g) * 0.5
    B = T * E
    a, lp_, v_, r_, ad_ = (torch.zeros(B, 2, device=DEV), torch.zeros(B, device=DEV), torch.zeros(B, device=DEV),
                           torch.zeros(B, device=DEV), torch.zeros(B, device=DEV))
    tr = _trainer(pol, val)
    mean_out = torch.empty(n, 2, device=DEV)
    value_out = torch.empty(n, 1, device=DEV)
    tr.minibatch(big, a, lp_, v_, r_, ad_, idx, mean_out=mean_out, value_out=value_out)
    rows = big[idx].contiguous()
    actor = RoverNet.from_state_dict(pol.state_dict(), final_act="tanh")
    critic = RoverNet.from_state_dict(val.state_dict(), final_act="none")
    assert torch.equal(mean_out, actor(rows)) and torch.equal(mean_out, tr.actor(rows))
    assert torch.equal(value_out, critic(rows)) and torch.equal(value_out, tr.critic(rows))


def _fused_grads(tr):
    from isaac_rover_orbit_amd.ppo import unpack
    g = tr.grad.cpu()
    pol = unpack(tr.desc_p, g[:tr.n_p])
    pol["log_std_parameter"] = g[tr.n_p + tr.n_v:tr.n_p + tr.n_v + 2]
    return {"policy": pol, "value": unpack(tr.desc_v, g[tr.n_p:tr.n_p + tr.n_v])}


@pytest.mark.parametrize("log_std", [(-0.4, 0.3), (2.5, -0.3), (2.0, -0.3)])
def test_gradients_match_float64_autograd(log_std):
    """Every weight, bias and log_std gradient is within 4x the error of torch fp32 autograd on the GPU (floor 1e-6 |g64|);
    the minibatch crosses both ratio clip branches with both signs of advantage, the value clip in both directions, and (second
    case) a log_std beyond the clamp, whose gradient is exactly 0, (third case) one exactly on the bound, inside the clamp as
    torch's clamp backward has it, whose gradient is not."""
    _gradient_case(4000, log_std)


@pytest.mark.parametrize("n,log_std", [pytest.param(n, ls, id=f"{n}-{name}") for n in (1, 5, 17, 4001)
                                       for name, ls in (("inside", (-0.4, 0.3)), ("beyond", (2.5, -0.3)))]
                         + [pytest.param(17, (2.0, -0.3), id="17-on_bound")])
def test_gradients_match_float64_autograd_at_ragged_rows(n, log_std):
    """The same bound at minibatches that end in a ragged group of 16 rows (the weight-gradient quads' row guard)."""
    _gradient_case(n, log_std)


def _gradient_case(n, log_std):
    ex, pol, val = _nets(0, log_std)
    obs, act, logp, oldv, ret, adv = _rollout(pol, val, 1, 4096, seed=3)
    idx = torch.randperm(4096, device=DEV)[:n].contiguous()
    if n == 4000:
        with torch.no_grad():
            mean = pol(obs[idx])
            ls = pol.log_std_parameter.clamp(-20.0, 2.0)
            r = ((-0.5 * ((act[idx] - mean) / ls.exp()) ** 2 - ls - 0.9189385332).sum(1) - logp[idx]).exp()
            dv = val(obs[idx])[:, 0] - oldv[idx]
        for lo_side in (r < 0.8, r > 1.2, (r >= 0.8) & (r <= 1.2)):
            assert int((lo_side & (adv[idx] > 0)).sum()) > 10 and int((lo_side & (adv[idx] < 0)).sum()) > 10
        assert int((dv > 0.2).sum()) > 10 and int((dv < -0.2).sum()) > 10
    tr = _trainer(pol, val)
    tr.minibatch(obs, act, logp, oldv, ret, adv, idx)
    fused = _fused_grads(tr)
    args = (obs[idx], act[idx], logp[idx], oldv[idx], ret[idx], adv[idx])
    _, _, g64 = loss_and_grads(pol.state_dict(), val.state_dict(), *args)
    pol.zero_grad(); val.zero_grad()
    loss, _ = ex.ppo_loss(pol, val, *args)
    loss.backward()
    t32 = {"policy": {k: p.grad for k, p in pol.named_parameters()}, "value": {k: p.grad for k, p in val.named_parameters()}}
    for role in ("policy", "value"):
        for k, ref in g64[role].items():
            ref = ref.cpu()
            e_f = float((fused[role][k].double() - ref).norm())
            e_t = float((t32[role][k].double().cpu() - ref).norm())
            assert e_f <= 4 * e_t + 1e-6 * float(ref.norm()), (role, k, e_f, e_t, float(ref.norm()))
    if log_std[0] > 2.0:
        assert fused["policy"]["log_std_parameter"][0] == 0.0
        if n == 4000:
            assert fused["policy"]["log_std_parameter"][1] != 0.0
    elif log_std[0] == 2.0:
        assert fused["policy"]["log_std_parameter"][0] != 0.0 and g64["policy"]["log_std_parameter"][0] != 0.0


def test_minibatch_and_update_are_deterministic():
    ex, pol, val = _nets(0)
    obs, act, logp, oldv, ret, adv = _rollout(pol, val, 2, 2048, seed=4)
    perms = [torch.randperm(4096, device=DEV) for _ in range(2)]
    outs = []
    for _ in range(2):
        tr = _trainer(pol, val)
        tr.minibatch(obs, act, logp, oldv, ret, adv, perms[0][:1000].contiguous())
        g = tr.grad.clone()
        kls, lr = tr.update(obs, act, logp, oldv, ret, adv, perms=perms, epochs=2, minibatches=4)
        outs.append((g, tr.params.clone(), kls, lr))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and outs[0][2:] == outs[1][2:]


def test_clip_and_adam_match_torch_in_float64():
    from isaac_rover_orbit_amd.ppo import pack
    ex, pol, val = _nets(0)
    lr = 1e-2
    tr = _trainer(pol, val, lr=lr)
    torch.manual_seed(9)
    gsd = {r: {k: torch.randn_like(p) * (0.05 if r == "policy" else 0.02) for k, p in net.named_parameters()}
           for r, net in (("policy", pol), ("value", val))}
    gp = pack(gsd["policy"], "tanh")[1]
    gv = pack(gsd["value"], "none")[1]
    gflat = torch.from_numpy(np.concatenate([gp, gv, gsd["policy"]["log_std_parameter"].numpy(), np.zeros(2, np.float32)])).to(DEV)
    ref_params = [p.detach().double().clone().requires_grad_(True) for net in (pol, val) for p in net.parameters()]
    ref_grads = [gsd[r][k].double() for r, net in (("policy", pol), ("value", val)) for k, _ in net.named_parameters()]
    opt = torch.optim.Adam(ref_params, lr=lr)
    p0 = tr.params.clone()
    for _ in range(3):
        tr.grad.copy_(gflat)
        tr.apply()
        for p, g in zip(ref_params, ref_grads):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(ref_params, 0.5)
        opt.step()
    sd = tr.state_dict()
    num = den = 0.0
    for (r, net) in (("policy", pol), ("value", val)):
        for k, p in net.named_parameters():
            ref = ref_params.pop(0).detach()
            d_ref = ref - p.detach().double()
            d_f = sd[r][k].double() - p.detach().double()
            num += float((d_f - d_ref).norm()) ** 2
            den += float(d_ref.norm()) ** 2
    assert num ** 0.5 <= 1e-5 * den ** 0.5, (num ** 0.5, den ** 0.5)
    assert tr.steps == 3
    pad = (p0 == 0) & (gflat == 0)
    assert torch.all(tr.params[pad] == 0) and torch.all(tr.adam_m[pad] == 0) and torch.all(tr.adam_v[pad] == 0)
    P, V = tr.n_p, tr.n_v
    for c in range(tr.n_copies):
        assert torch.equal(tr.rep_p[c * P:(c + 1) * P], tr.params[:P])
        assert torch.equal(tr.rep_v[c * V:(c + 1) * V], tr.params[P:P + V])


def test_gae_bit_identical_to_the_example_loop():
    ex, pol, val = _nets(0)
    tr = _trainer(pol, val)
    T, n = 60, 4096
    g = torch.Generator(device=DEV).manual_seed(7)
    rew = torch.randn(T, n, device=DEV, generator=g)
    done = (torch.rand(T, n, device=DEV, generator=g) < 0.05).float()
    vals = torch.randn(T, n, device=DEV, generator=g)
    last_v = torch.randn(n, device=DEV, generator=g)
    gamma, lam = ex.GAMMA, ex.LAM
    adv = torch.zeros_like(rew); gae = torch.zeros(n, device=DEV)
    for t in reversed(range(T)):                               # examples/04_train_ppo.py, verbatim
        nv = last_v if t == T - 1 else vals[t + 1]
        nd = 1.0 - done[t]
        delta = rew[t] + gamma * nv * nd - vals[t]
        gae = delta + gamma * lam * nd * gae
        adv[t] = gae
    ret = adv + vals
    a2, r2 = tr.gae(rew, done, vals, last_v)
    assert int(done.sum()) > 1000
    assert torch.equal(a2, adv) and torch.equal(r2, ret)


def test_one_update_tracks_the_example_torch_update():
    _track_the_example_update(512, 8, 2, 4)


def test_update_with_unequal_minibatches_tracks_the_example():
    """B = 4100 rows in 3 minibatches: perm.chunk(3) gives 1367, 1367 and 1366 rows, none a multiple of 16."""
    _track_the_example_update(1025, 4, 2, 3)


def _track_the_example_update(n_env, T, epochs, mbs):
    ex, pol, val = _nets(0)
    obs, act, logp, oldv, ret, adv = _rollout(pol, val, T, n_env, seed=8, lp_noise=0.15, v_noise=0.3)
    B = T * n_env
    perms = [torch.randperm(B, device=DEV) for _ in range(epochs)]
    tr = _trainer(pol, val)
    p0 = {r: {k: v.detach().cpu().clone() for k, v in sd.items()} for r, sd in (("policy", pol.state_dict()), ("value", val.state_dict()))}
    kls_f, lr_f = tr.update(obs, act, logp, oldv, ret, adv, perms=perms, epochs=epochs, minibatches=mbs)
    # the example's torch update on the same data and permutations
    pol, val = pol.to(DEV), val.to(DEV)
    opt = torch.optim.Adam(list(pol.parameters()) + list(val.parameters()), lr=1e-4)
    kls_t = []
    for e in range(epochs):
        kls = []
        for mb in perms[e].chunk(mbs):
            loss, kl = ex.ppo_loss(pol, val, obs[mb], act[mb], logp[mb], oldv[mb], ret[mb], adv[mb])
            kls.append(kl)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(list(pol.parameters()) + list(val.parameters()), 0.5)
            opt.step()
        kl_mean = torch.stack(kls).mean().item()
        lr = opt.param_groups[0]["lr"]
        if kl_mean > 2 * ex.KL_THR: lr = max(lr / 1.5, 1e-6)
        elif kl_mean < 0.5 * ex.KL_THR: lr = min(lr * 1.5, 1e-2)
        for g in opt.param_groups: g["lr"] = lr
        kls_t.append(kl_mean)
    assert lr_f == pytest.approx(opt.param_groups[0]["lr"], rel=1e-12)
    for a, b in zip(kls_f, kls_t):
        assert a == pytest.approx(b, rel=1e-3)
    sd = tr.state_dict()
    num = den = 0.0
    for r, net in (("policy", pol), ("value", val)):
        for k, p in net.state_dict().items():
            d_t = p.double().cpu() - p0[r][k].double()
            d_f = sd[r][k].double() - p0[r][k].double()
            num += float((d_f - d_t).norm()) ** 2
            den += float(d_t.norm()) ** 2
    assert num ** 0.5 <= 0.05 * den ** 0.5, (num ** 0.5, den ** 0.5)


def test_state_dict_export_reproduces_the_trainer_actor():
    from isaac_rover_orbit_amd.policy import RoverNet
    ex, pol, val = _nets(0)
    obs, act, logp, oldv, ret, adv = _rollout(pol, val, 1, 1024, seed=2)
    tr = _trainer(pol, val)
    tr.update(obs, act, logp, oldv, ret, adv, epochs=1, minibatches=2)
    sd = tr.state_dict()
    rows = obs[:333].contiguous()
    assert torch.equal(RoverNet.from_state_dict(sd["policy"], final_act="tanh")(rows), tr.actor(rows))
    assert torch.equal(RoverNet.from_state_dict(sd["value"], final_act="none")(rows), tr.critic(rows))
    net = ex.Net(2, True)
    net.load_state_dict(sd["policy"])                          # loads into the example's module as well


def test_refusals_return_documented_codes():
    from isaac_rover_orbit_amd import _lib
    ex, pol, val = _nets(0)
    obs, act, logp, oldv, ret, adv = _rollout(pol, val, 1, 64, seed=2)
    tr = _trainer(pol, val)
    lib = _lib.load()
    idx = torch.arange(64, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    stats = torch.empty(4, device=DEV)

    def call(dp, n, ws_bytes):
        return lib.rover_ppo_minibatch(C.byref(dp), C.byref(tr.desc_v), C.byref(tr.hp), tr.params.data_ptr(), obs.data_ptr(),
                                       act.data_ptr(), logp.data_ptr(), oldv.data_ptr(), ret.data_ptr(), adv.data_ptr(),
                                       idx.data_ptr(), n, tr.ws.data_ptr(), ws_bytes, tr.grad.data_ptr(), stats.data_ptr(),
                                       None, None, s)
    need = lib.rover_ppo_workspace_bytes(64)
    tr._ensure_ws(64)
    assert call(tr.desc_p, 64, need) == 0
    bad = _lib.PolicyDesc.from_buffer_copy(tr.desc_p)
    bad.layers[1].N = 64
    assert call(bad, 64, need) == 4                                  # ROVER_ERR_UNSUPPORTED
    assert call(tr.desc_p, 0, need) == 1 and call(tr.desc_p, -3, need) == 1   # ROVER_ERR_INVALID
    assert call(tr.desc_p, 64, need - 4) == 1
    torch.cuda.synchronize()
