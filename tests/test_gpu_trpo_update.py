"""Fused TRPO update on the MI355X (include/rover_trpo.h, isaac_rover_orbit_amd.trpo) against the torch spec: surrogate gradient,
Fisher-vector products, the CG solution and the value regression agree with float64 as closely as torch fp32 does on the same
inputs; the step and the accepted trial equal the spec's; runs are bit-reproducible; a rejected search restores everything."""
import pytest
import torch

from trpo_helpers import DEV, _check, _copy, _err, _flat_to_sd, _nets, _rollout, _spec_step, _trainer

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("log_std", [(-0.4, 0.3), (2.5, -0.3)])
def test_surrogate_gradient_matches_float64(log_std):
    from isaac_rover_orbit_amd.trpo import surrogate_loss
    pol, val = _nets(0, log_std)
    obs, act, logp, ret, adv = _rollout(pol, 60 * 256)
    tr = _trainer(pol, val)
    g = tr.unvector(tr.policy_grad(obs, act, logp, adv).clone())
    ref = {}
    for dt in (torch.float64, torch.float32):
        p = _copy(pol, dt)
        gr = torch.autograd.grad(surrogate_loss(p, obs.to(dt), act.to(dt), logp.to(dt), adv.to(dt)), list(p.parameters()))
        ref[dt] = dict(zip([k for k, _ in p.named_parameters()], gr))
    _check(g, ref[torch.float64], ref[torch.float32])
    if log_std[0] > 2.0:
        assert g["log_std_parameter"][0] == 0.0 and g["log_std_parameter"][1] != 0.0
    assert torch.count_nonzero(tr.grad[tr.n_p:tr.n_p + tr.n_v]) == 0


@pytest.mark.parametrize("log_std", [(-0.4, 0.3), (2.5, -0.3)])
def test_fvp_matches_float64(log_std):
    from isaac_rover_orbit_amd.trpo import fisher_vector_product
    pol, val = _nets(0, log_std)
    obs, act, logp, ret, adv = _rollout(pol, 60 * 256, seed=2)
    tr = _trainer(pol, val)
    tr.policy_grad(obs, act, logp, adv)
    gen = torch.Generator().manual_seed(5)
    for _ in range(2):
        vsd = {k: torch.randn(p.shape, generator=gen) for k, p in pol.named_parameters()}
        out = tr.unvector(tr.fvp(obs, tr.vector(vsd)))
        ref = {}
        for dt in (torch.float64, torch.float32):
            p = _copy(pol, dt)
            v = torch.cat([vsd[k].reshape(-1) for k, _ in p.named_parameters()]).to(DEV, dt)
            ref[dt] = _flat_to_sd(p, fisher_vector_product(p, obs.to(dt), v, 0.1).detach())
        _check(out, ref[torch.float64], ref[torch.float32])


def test_policy_step_matches_spec():
    """CG solution within 4x torch fp32's error (floor 1e-3 |x|), step and xHx to 1e-3, the same accepted trial and CG count."""
    pol, val = _nets(1)
    obs, act, logp, ret, adv = _rollout(pol, 60 * 256, seed=3)
    tr = _trainer(pol, val)
    g_out, x_out = torch.empty_like(tr.params), torch.empty_like(tr.params)
    tr.policy_step(obs, act, logp, adv, grad_out=g_out, dir_out=x_out)
    s = tr.stats()
    p64, st64 = _spec_step(pol, val, obs, act, logp, adv, torch.float64)
    p32, st32 = _spec_step(pol, val, obs, act, logp, adv, torch.float32)
    _check(tr.unvector(x_out), _flat_to_sd(p64, st64["direction"]), _flat_to_sd(p32, st32["direction"]), floor=1e-3)
    assert s["cg_iters"] == st64["cg_iters"]
    assert s["xhx"] == pytest.approx(st64["xhx"], rel=1e-3) and s["step"] == pytest.approx(st64["step"], rel=1e-3)
    assert s["accepted"] == st64["accepted"] >= 0
    assert s["kl"] == pytest.approx(st64["kl"], rel=2e-2) and s["loss_old"] == pytest.approx(st64["loss_old"], rel=1e-4, abs=1e-6)
    sd = tr.state_dict()["policy"]
    for k, ref in p64.state_dict().items():
        assert _err(sd[k], ref) <= 1e-3 * float(ref.norm()) + 1e-6, k


def test_value_minibatch_clip_and_adam_match_float64():
    from isaac_rover_orbit_amd.trpo import HPARAMS
    pol, val = _nets(2)
    obs, act, logp, ret, adv = _rollout(pol, 60 * 256, seed=4)
    tr = _trainer(pol, val)
    idx = torch.randperm(60 * 256, device=DEV)[:256].contiguous()
    tr.value_minibatch(obs, ret, idx)
    g = tr.grad[tr.n_p:tr.n_p + tr.n_v].clone()
    from isaac_rover_orbit_amd.ppo import unpack
    g_sd = unpack(tr.desc_v, g)
    ref, nets = {}, {}
    for dt in (torch.float64, torch.float32):
        v = _copy(val, dt)
        loss = torch.nn.functional.mse_loss(ret[idx].to(dt), v(obs[idx].to(dt)).squeeze(1))
        loss.backward()
        ref[dt] = {k: p.grad.clone() for k, p in v.named_parameters()}
        nets[dt] = (v, float(loss))
    _check(g_sd, ref[torch.float64], ref[torch.float32])
    assert tr.stats()["value_loss_sum"] == pytest.approx(nets[torch.float64][1], rel=1e-5)
    tr.value_apply()
    v64 = nets[torch.float64][0]
    torch.nn.utils.clip_grad_norm_(v64.parameters(), HPARAMS["grad_norm_clip"])
    torch.optim.Adam(v64.parameters(), lr=HPARAMS["value_learning_rate"]).step()
    st = tr.stats()
    assert st["value_step"] == 1 and st["clip_coef"] <= 1.0
    new = tr.state_dict()["value"]
    for k, p in v64.named_parameters():
        # one Adam step moves every weight by ~lr; agreement to 1 % of lr per element
        assert float((new[k].double() - p.detach().cpu()).abs().max()) <= 1e-2 * HPARAMS["value_learning_rate"], k
    x = obs[:64].contiguous()
    assert torch.equal(tr.critic(x), __import__("isaac_rover_orbit_amd.policy", fromlist=["RoverNet"]).RoverNet.from_state_dict(
        new, final_act="none")(x))


def test_update_is_bit_reproducible():
    pol, val = _nets(3)
    B = 60 * 256
    obs, act, logp, ret, adv = _rollout(pol, B, seed=5)
    perms = [torch.randperm(B, device=DEV) for _ in range(4)]
    outs = []
    for _ in range(2):
        tr = _trainer(pol, val)
        st = tr.update(obs, act, logp, ret, adv, perms=perms)
        outs.append((tr.params.clone(), tr.rep_p.clone(), tr.rep_v.clone(), st))
    assert all(torch.equal(a, b) for a, b in zip(outs[0][:3], outs[1][:3]))
    assert outs[0][3] == outs[1][3]


def test_forced_restore_leaves_parameters_and_replicas_unchanged():
    pol, val = _nets(4)
    obs, act, logp, ret, adv = _rollout(pol, 60 * 256, seed=6)
    tr = _trainer(pol, val, max_kl=1e-30)
    before = (tr.params.clone(), tr.rep_p.clone())
    tr.policy_step(obs, act, logp, adv)
    s = tr.stats()
    assert s["accepted"] == -1 and s["trials"] == 10
    assert torch.equal(tr.params, before[0]) and torch.equal(tr.rep_p, before[1])


def test_state_dict_round_trips_into_rovernet():
    from isaac_rover_orbit_amd.policy import RoverNet
    pol, val = _nets(5)
    obs, act, logp, ret, adv = _rollout(pol, 60 * 256, seed=7)
    tr = _trainer(pol, val)
    tr.update(obs, act, logp, ret, adv)
    sd = tr.state_dict()
    x = obs[:300].contiguous()
    assert torch.equal(RoverNet.from_state_dict(sd["policy"], final_act="tanh")(x), tr.actor(x))
    assert torch.equal(RoverNet.from_state_dict(sd["value"], final_act="none")(x), tr.critic(x))
    tr2 = type(tr).from_checkpoint(sd)
    assert torch.equal(tr2.params, tr.params)


def test_full_size_update_tracks_the_spec():
    """One whole update at 60 x 4096 rows: the same accepted trial and CG count as the torch fp32 spec, KL and step close."""
    from isaac_rover_orbit_amd.trpo import TorchTRPO
    pol, val = _nets(6)
    B = 60 * 4096
    obs, act, logp, ret, adv = _rollout(pol, B, seed=8)
    perms = [torch.randperm(B, device=DEV) for _ in range(4)]
    tr = _trainer(pol, val)
    st = tr.update(obs, act, logp, ret, adv, perms=perms)
    p32, v32 = _copy(pol, torch.float32), _copy(val, torch.float32)
    ref = TorchTRPO(p32, v32).update(obs, act, logp, ret, adv, perms=perms)
    assert st["accepted"] == ref["accepted"] >= 0
    assert st["step"] == pytest.approx(ref["step"], rel=2e-2) and st["kl"] == pytest.approx(ref["kl"], rel=5e-2)
    assert st["value_loss"] == pytest.approx(ref["value_loss"], rel=2e-2)
