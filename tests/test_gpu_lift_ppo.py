"""Fused lift PPO update on the MI355X (include/rover_lift_train.h, isaac_rover_orbit_amd.lift_ppo) against the torch spec
(TorchLiftPPO) and float64: the ELU forward, the RunningStandardScaler, the training forward's bit identity with the inference
forward, gradients, the KL early stop, a whole 8 x 24 update, determinism, refusals and the example end to end."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lift_ppo_reference import NumpyScaler, loss_and_grads, net_forward

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nets(seed=0, log_std=None):
    from isaac_rover_orbit_amd import lift_ppo as LP
    torch.manual_seed(seed)
    pol, val = LP.LiftMLP(8, log_std=True), LP.LiftMLP(1)
    if log_std is not None:
        with torch.no_grad():
            pol.log_std_parameter.copy_(torch.as_tensor(log_std, dtype=torch.float32))
    return pol.to(DEV), val.to(DEV)


def _rollout(pol, val, B, seed=1, lp_noise=0.3, v_noise=0.4, scale=1.0):
    """Synthetic flat rollout (B rows): raw states, actions, logp / values of the networks on the initially standardised states
    (+ noise so that the ratios and value errors cross every clip branch), returns, advantages."""
    from isaac_rover_orbit_amd import lift_ppo as LP
    g = torch.Generator(device=DEV).manual_seed(seed)
    obs = torch.randn(B, 36, device=DEV, generator=g) * scale
    sc = LP.RunningStandardScaler(36, device=DEV)
    with torch.no_grad():
        s = sc(obs)
        mean, v0 = pol(s), val(s)[:, 0]
        act = mean + pol.log_std_parameter.clamp(-20, 2).exp() * torch.randn(B, 8, device=DEV, generator=g)
        lp = LP.gaussian_logp(mean, pol.log_std_parameter, act)
    logp = (lp + lp_noise * torch.randn(B, device=DEV, generator=g)).contiguous()
    oldv = (v0 + v_noise * torch.randn(B, device=DEV, generator=g)).contiguous()
    ret = (oldv + torch.randn(B, device=DEV, generator=g)).contiguous()
    adv = torch.randn(B, device=DEV, generator=g)
    return obs.contiguous(), act.contiguous(), logp, oldv, ret, adv


def _trainer(pol, val, **kw):
    from isaac_rover_orbit_amd.lift_ppo import FusedLiftPPO
    return FusedLiftPPO(pol.state_dict(), val.state_dict(), **kw)


@pytest.mark.parametrize("n", [1, 17, 4101])
def test_elu_forward_matches_float64(n):
    from isaac_rover_orbit_amd import lift_ppo as LP
    pol, val = _nets(3)
    x = torch.randn(n, 36, device=DEV) * 2.0
    for net in (pol, val):
        hip = LP.lift_net(net.state_dict())(x)
        ref = net_forward({k: v.double() for k, v in net.state_dict().items()}, x.double())
        err = (hip.double() - ref).abs().max().item()
        assert err <= 1e-5 * max(1.0, ref.abs().max().item()), err
        assert (hip - net(x)).abs().max().item() <= 2e-5


def test_standardize_bit_identical_and_statistics_match_float64():
    from isaac_rover_orbit_amd import lift_ppo as LP
    pol, val = _nets(0)
    tr = _trainer(pol, val)
    ts, ns = LP.RunningStandardScaler(36, device=DEV), NumpyScaler(36)
    g = torch.Generator(device=DEV).manual_seed(4)
    for i in range(4):
        x = (torch.randn(1000 + 77 * i, 36, device=DEV, generator=g) * (1 + 3 * i) + i).contiguous()
        x[0, 0], x[0, 1] = 1e4, -1e4                                  # outside the clamp
        out = tr.standardize(x, "state", train=True)
        ns.train(x.double().cpu().numpy())
        ts(x, train=True)
        blk = tr.state_scaler.cpu().numpy()
        np.testing.assert_allclose(blk[:36], ns.mean, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(blk[36:72], ns.var, rtol=1e-12)
        assert blk[72] == ns.count
        # the torch expression on the SAME scaler state gives the same bits
        mean, var = tr.state_scaler[:36], tr.state_scaler[36:72]
        expect = torch.clamp((x - mean.float()) / (torch.sqrt(var.float()) + 1e-8), min=-5.0, max=5.0)
        assert torch.equal(out, expect)
        y = torch.randn(333, 36, device=DEV, generator=g) * 4
        inv = tr.standardize(y, "state", inverse=True)
        assert torch.equal(inv, torch.sqrt(var.float()) * torch.clamp(y, min=-5.0, max=5.0) + mean.float())
        # the torch scaler (float32 batch statistics) tracks float64
        np.testing.assert_allclose(ts.running_mean.cpu().numpy(), ns.mean, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(ts.running_variance.cpu().numpy(), ns.var, rtol=1e-4)
    v = torch.randn(5000, device=DEV, generator=g) * 3 + 1
    tr.standardize(v.reshape(-1, 1), "value", train=True)
    nv = NumpyScaler(1)
    nv.train(v.double().cpu().numpy().reshape(-1, 1))
    np.testing.assert_allclose(tr.value_scaler.cpu().numpy(), [nv.mean[0], nv.var[0], nv.count], rtol=1e-12)


@pytest.mark.parametrize("n", [1, 16, 17, 4096])
def test_training_forward_is_bit_identical_to_the_inference_forward(n):
    pol, val = _nets(1, log_std=torch.linspace(-0.6, 0.3, 8))
    B = 24 * 512
    obs, act, logp, oldv, ret, adv = _rollout(pol, val, B, scale=3.0)
    tr = _trainer(pol, val)
    tr.standardize(obs[:4000], "state", train=True)                  # a non-trivial scaler state
    g = torch.Generator(device=DEV).manual_seed(n)
    idx = torch.randint(0, B, (n,), device=DEV, generator=g)
    mean_out = torch.empty(n, 8, device=DEV)
    value_out = torch.empty(n, 1, device=DEV)
    tr.minibatch(obs, act, logp, oldv, ret, adv, idx, mean_out=mean_out, value_out=value_out)
    rows = tr.standardize(obs[idx].contiguous(), "state")
    assert torch.equal(mean_out, tr.actor(rows)) and torch.equal(value_out, tr.critic(rows))
    from isaac_rover_orbit_amd import lift_ppo as LP
    assert torch.equal(mean_out, LP.lift_net(pol.state_dict())(rows))


def _grads_of(tr):
    from isaac_rover_orbit_amd import lift_ppo as LP
    g = tr.grad.cpu()
    pol = LP.unpack(tr.desc_p, g[:tr.n_p])
    pol["log_std_parameter"] = g[tr.n_p + tr.n_v:].clone()
    return {"policy": pol, "value": LP.unpack(tr.desc_v, g[tr.n_p:tr.n_p + tr.n_v])}


@pytest.mark.parametrize("log_std", [[-0.5, 0.2, 0.0, -1.0, 0.4, -0.2, 0.1, 2.5]])
def test_gradients_match_float64_autograd(log_std):
    _gradient_case(4096, log_std)


@pytest.mark.parametrize("n", [1, 17, 4099])
def test_gradients_match_float64_autograd_at_ragged_rows(n):
    """The same bound at minibatches that end in a ragged 16-row workgroup; the clamped log_std's gradient stays exactly 0."""
    _gradient_case(n, [-0.5, 0.2, 0.0, -1.0, 0.4, -0.2, 0.1, 2.5])


def _gradient_case(n, log_std):
    from isaac_rover_orbit_amd import lift_ppo as LP
    pol, val = _nets(2, log_std=log_std)                              # log_std[7] = 2.5: clamped, no gradient
    B = 8192
    obs, act, logp, oldv, ret, adv = _rollout(pol, val, B, seed=3)
    tr = _trainer(pol, val)
    idx = torch.randperm(B, device=DEV)[:n].contiguous()
    tr.minibatch(obs, act, logp, oldv, ret, adv, idx)
    s = tr.standardize(obs[idx].contiguous(), "state")
    if n == 4096:
        with torch.no_grad():                                         # every clip branch is crossed
            lp = LP.gaussian_logp(pol(s), pol.log_std_parameter, act[idx])
            r = (lp - logp[idx]).exp()
            dv = val(s)[:, 0] - oldv[idx]
        for side in (r < 0.8, r > 1.2):
            assert int((side & (adv[idx] > 0)).sum()) > 10 and int((side & (adv[idx] < 0)).sum()) > 10
        assert int((dv > 0.2).sum()) > 10 and int((dv < -0.2).sum()) > 10
    args = (s, act[idx], logp[idx], oldv[idx], ret[idx], adv[idx])
    _, _, ref = loss_and_grads(pol.state_dict(), val.state_dict(), *args)
    _, _, t32 = loss_and_grads(pol.state_dict(), val.state_dict(), *args, dtype=torch.float32)
    fused = _grads_of(tr)
    for role in ("policy", "value"):
        for k, g64 in ref[role].items():
            g64 = g64.cpu()
            e_f = float((fused[role][k].double() - g64).norm())
            e_t = float((t32[role][k].double().cpu() - g64).norm())
            assert e_f <= 4 * e_t + 1e-6 * float(g64.norm()), (role, k, e_f, e_t, float(g64.norm()))
    assert fused["policy"]["log_std_parameter"][7] == 0.0
    if n == 4096:
        assert fused["policy"]["log_std_parameter"][0] != 0.0


def test_kl_early_stop_skips_the_rest_of_the_epoch():
    pol, val = _nets(4)
    B = 4096
    obs, act, logp, oldv, ret, adv = _rollout(pol, val, B, seed=5, lp_noise=0.5)   # KL ~ 0.1 > 0.008
    tr = _trainer(pol, val)
    perm = torch.randperm(B, device=DEV)
    mbs = [c.contiguous() for c in perm.chunk(8)]
    stats = torch.full((8, 4), -7.0, device=DEV)
    tr.standardize(obs[:1000], "state", train=True)
    snap = lambda: [t.clone() for t in (tr.params, tr.adam_m, tr.adam_v, tr.state_scaler, tr.rep_p, tr.rep_v)]  # noqa: E731
    before = snap()
    tr.minibatch(obs, act, logp, oldv, ret, adv, mbs[0], train_scaler=False, stats=stats[0])
    tr.apply()                                                        # skipped: skrl breaks before the optimiser step
    after = snap()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert tr.steps == 0 and tr._word(7) == 1 and tr._word(8) == 1
    kl0 = stats[0, 0].item()
    assert kl0 > 0.008
    grad0 = tr.grad.clone()
    for j in range(1, 4):                                             # the rest of the epoch does nothing, scaler training included
        tr.minibatch(obs, act, logp, oldv, ret, adv, mbs[j], train_scaler=True, stats=stats[j])
        tr.apply()
    assert all(torch.equal(a, b) for a, b in zip(before, snap())) and torch.equal(tr.grad, grad0)
    assert torch.all(stats[1:] == -7.0) and tr._word(8) == 1
    kl = torch.empty(1, device=DEV)
    tr.kl_schedule(stats[:4], kl)
    assert kl.item() == kl0                                           # the epoch's mean counts up to the stopping minibatch
    assert tr.lr == pytest.approx(1e-4 / 1.5, rel=1e-12)               # kl > 2 x 0.008
    assert tr._word(7) == 0 and tr._word(8) == 0 and tr.stopped_epochs == 1
    tr.hp.kl_early_stop = 0.0                                         # next epoch resumes (and, with the stop off, steps)
    tr.minibatch(obs, act, logp, oldv, ret, adv, mbs[1], stats=stats[1])
    tr.apply()
    assert tr.steps == 1 and not torch.equal(tr.params, before[0]) and stats[1, 0].item() != -7.0


@pytest.mark.parametrize("lr,kl_stop", [(1e-4, 0.0), (1e-3, 0.008)])
def test_whole_update_tracks_the_torch_spec(lr, kl_stop):
    from isaac_rover_orbit_amd import lift_ppo as LP
    pol, val = _nets(0)
    B = 24 * 128
    data = _rollout(pol, val, B, seed=5, lp_noise=0.0, v_noise=0.3)
    g = torch.Generator(device=DEV).manual_seed(9)
    perms = [torch.randperm(B, device=DEV, generator=g) for _ in range(8)]
    tr = _trainer(pol, val, lr=lr, kl_early_stop=kl_stop)
    p0 = {r: {k: v.detach().cpu().clone() for k, v in sd.items()} for r, sd in (("policy", pol.state_dict()), ("value", val.state_dict()))}
    kls_f, lr_f = tr.update(*data, perms=perms)
    spec = LP.TorchLiftPPO(pol, val, lr=lr, kl_early_stop=kl_stop)
    kls_t, lr_t = spec.update(*data, perms=perms)
    assert tr.stopped_epochs == spec.stopped_epochs
    assert (kl_stop == 0.0) == (spec.stopped_epochs == 0)
    assert lr_f == pytest.approx(lr_t, rel=1e-12)
    for a, b in zip(kls_f, kls_t):
        assert a == pytest.approx(b, rel=2e-3, abs=1e-6)
    np.testing.assert_allclose(tr.state_scaler[:36].cpu().numpy(), spec.state_preprocessor.running_mean.cpu().numpy(), rtol=1e-5, atol=1e-6)
    sd = tr.state_dict()
    num = den = 0.0
    for r, net in (("policy", pol), ("value", val)):
        for k, p in net.state_dict().items():
            d_t = p.double().cpu() - p0[r][k].double()
            d_f = sd[r][k].double() - p0[r][k].double()
            num += float((d_f - d_t).norm()) ** 2
            den += float(d_t.norm()) ** 2
    assert den > 0 and num ** 0.5 <= 0.05 * den ** 0.5, (num ** 0.5, den ** 0.5)


def test_update_is_deterministic():
    pol, val = _nets(6)
    B = 24 * 64
    data = _rollout(pol, val, B, seed=7, lp_noise=0.05)
    perms = [torch.randperm(B, device=DEV) for _ in range(8)]
    outs = []
    for _ in range(2):
        tr = _trainer(pol, val)
        kls, lr = tr.update(*data, perms=perms)
        outs.append((tr.params.clone(), tr.adam_v.clone(), tr.state_scaler.clone(), kls, lr, tr.steps))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    assert outs[0][3:] == outs[1][3:]


def test_checkpoint_round_trip_and_refusals():
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd import lift_ppo as LP
    pol, val = _nets(8)
    tr = _trainer(pol, val)
    x = torch.randn(500, 36, device=DEV)
    tr.standardize(x, "state", train=True)
    ck = tr.state_dict()
    assert set(ck) == {"policy", "value", "state_preprocessor", "value_preprocessor"}
    tr2 = LP.FusedLiftPPO.from_checkpoint(ck)
    assert torch.equal(tr2.params, tr.params) and torch.equal(tr2.state_scaler, tr.state_scaler)
    rows = tr.standardize(x, "state")
    assert torch.equal(tr2.actor(rows), tr.actor(rows))
    lib = _lib.load()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    idx = torch.arange(64, device=DEV)
    stats = torch.zeros(4, device=DEV)
    tr._ensure_ws(64)
    need = int(lib.rover_lift_ppo_workspace_bytes(64))
    assert tr.ws.numel() >= need
    call = lambda dp, dv, n, wsb: lib.rover_lift_ppo_minibatch(  # noqa: E731
        C.byref(dp), C.byref(dv), C.byref(tr.hp), tr.params.data_ptr(), tr.state_scaler.data_ptr(), x.data_ptr(), x.data_ptr(),
        x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), idx.data_ptr(), n, 0, tr.state.data_ptr(), tr.ws.data_ptr(), wsb,
        tr.grad.data_ptr(), stats.data_ptr(), None, None, s)
    assert call(tr.desc_p, tr.desc_v, 64, need) == 0
    rp, rv = _lib.PolicyDesc(), _lib.PolicyDesc()
    lib.rover_policy_default_desc(C.byref(rp), 2, 1)
    lib.rover_policy_default_desc(C.byref(rv), 1, 0)
    assert call(rp, rv, 64, need) == 4                                # ROVER_ERR_UNSUPPORTED: the rover pair
    assert call(tr.desc_v, tr.desc_p, 64, need) == 4
    assert call(tr.desc_p, tr.desc_v, 0, need) == 1 and call(tr.desc_p, tr.desc_v, 64, need - 4) == 1   # ROVER_ERR_INVALID
    torch.cuda.synchronize()


def test_example_trains_end_to_end(tmp_path):
    out = tmp_path / "curve.jsonl"
    ck = tmp_path / "ck.pt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "05_train_lift.py"), "--update", "fused", "--iterations", "2",
                        "--num_envs", "256", "--out", str(out), "--save", str(ck)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    assert len(lines) == 2 and all(np.isfinite(l["kl"]) and l["lr"] > 0 for l in lines)
    assert "Episode Reward/lifting_object" in lines[0]
    sd = torch.load(ck, map_location="cpu", weights_only=False)
    assert sd["policy"]["net.0.weight"].shape == (256, 36) and sd["state_preprocessor"]["current_count"] > 1
