"""Rover PPO behind skrl's running scalers on the MI355X (isaac_rover_orbit_amd.ppo_scaled / rollout_scaled): the collector's three
launches against their parts, and FusedScaledPPO.update against TorchScaledPPO.update at the bounds tests/test_gpu_ppo_update.py
holds the unscaled update to."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from lift_ppo_reference import NumpyScaler
from rollout_helpers import _biteq, _inject, make_nets, run_all, synthetic_rows
from test_gpu_ppo_update import _nets, _rollout

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLT_MAX = float(np.finfo(np.float32).max)


# ------------------------------------------------------------------------------------------------------------------ collector
def _sanitise(raw):
    return torch.nan_to_num(raw, nan=0.0, posinf=FLT_MAX, neginf=0.0)


@pytest.mark.parametrize("n", [1, 17, 100])
def test_collector_is_its_three_launches(n):
    from isaac_rover_orbit_amd.policy import forward_pair
    from isaac_rover_orbit_amd.rollout_scaled import ScaledRolloutCollector
    from isaac_rover_orbit_amd.scaler import DeviceScaler
    T = 3
    nets = make_nets(2)
    log_std = torch.tensor([-0.4, 0.3], device=DEV)
    ss, vs = DeviceScaler(965, DEV), DeviceScaler(1, DEV)
    g = torch.Generator(device=DEV).manual_seed(n)
    ss.train(_sanitise(synthetic_rows(300, seed=50)).contiguous())
    vs.train((torch.randn(400, 1, device=DEV, generator=g) * 6 - 2).contiguous())
    col = ScaledRolloutCollector(nets[0], nets[1], log_std, ss, vs, n, T)
    for t in range(T):
        raw = _inject(synthetic_rows(max(n, 17), seed=t), max(n, 17))[:n].contiguous()
        assert bool(torch.isinf(raw).any()) and bool((raw == float("-inf")).any())      # the scanner's miss is among the inputs
        if t == 2:          # a scaler update between two steps, seen without rebuilding the collector
            before = ss.forward(_sanitise(raw))
            ss.train((_sanitise(synthetic_rows(200, seed=60)) * 2 + 0.3).contiguous())
            vs.train((torch.randn(100, 1, device=DEV, generator=g) + 4).contiguous())
        env_act = col.act(t, raw).clone()
        san = _sanitise(raw)
        assert _biteq(col.obs[t], san)
        s = ss.forward(san)
        assert _biteq(col.states, s)
        if t == 2:
            assert not torch.equal(s, before)
        mean, v = forward_pair(nets[0], nets[1], s)
        assert _biteq(col.mean[t], mean) and _biteq(col.val_s, v)
        assert _biteq(col.val[t], vs.inverse(v).reshape(n))
        blk = vs.block
        assert _biteq(col.val[t], (torch.sqrt(blk[1:2].float()) * torch.clamp(v, min=-5.0, max=5.0) + blk[0:1].float()).reshape(n))
        direct = run_all(nets, s, log_std, counter=t)                                     # rollout_act on the standardised rows
        assert _biteq(direct["obs"], s)                                                   # its nan_to_num is the identity there
        assert _biteq(col.actions[t], direct["act"]) and _biteq(env_act, direct["env_act"]) and _biteq(col.logp[t], direct["logp"])
        assert _biteq(col.mean[t], direct["mean"]) and _biteq(col.val_s, direct["val"])
        assert col.counter == t + 1
    lv = col.last_value(raw)
    assert col.counter == T and _biteq(lv, col.val[T - 1])
    assert col.state_dict() == {"seed": 42, "counter": T, "env_id_offset": 0}


# --------------------------------------------------------------------------------------------------------------------- update
class _Doubled(nn.Module):
    """net(2 x): `_rollout` draws rows of standard deviation 0.5 and asks the networks for the old log-probabilities and values
    on them; the standardised rows the update feeds the networks are those rows over 0.5 (up to the sample statistics)."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    @property
    def log_std_parameter(self):
        return self.net.log_std_parameter

    def forward(self, x):
        return self.net(2.0 * x)


def _inputs(pol, val, T, n_env, seed=8):
    """`_rollout` of tests/test_gpu_ppo_update.py, its observations scaled and offset per column (scales 0.2 .. 4.2, offsets
    -3 .. 3): a scaler far from the identity, whose output is close to the rows the old log-probabilities were taken on."""
    obs, act, logp, oldv, ret, adv = _rollout(_Doubled(pol), _Doubled(val), T, n_env, seed=seed, lp_noise=0.15, v_noise=0.3)
    g = torch.Generator(device=DEV).manual_seed(seed + 100)
    col = torch.rand(965, device=DEV, generator=g)
    raw = (obs * (0.2 + 4.0 * col) + (col - 0.5) * 6.0).contiguous()
    oldv, ret = (oldv * 3.0 + 5.0).contiguous(), (ret * 3.0 + 5.0).contiguous()        # a value scaler far from the identity too
    return raw, act, logp, oldv, ret, adv


def _step_error(sd_a, sd_b, p0):
    num = den = 0.0
    for r in ("policy", "value"):
        for k, p in sd_b[r].items():
            d_b = p.double().cpu() - p0[r][k].double()
            d_a = sd_a[r][k].double().cpu() - p0[r][k].double()
            num += float((d_a - d_b).norm()) ** 2
            den += float(d_b.norm()) ** 2
    return num ** 0.5, den ** 0.5


def _check_bounds(kls_a, lr_a, sd_a, kls_b, lr_b, sd_b, p0):
    """tests/test_gpu_ppo_update.py:253-264: lr rel 1e-12, epoch KLs rel 1e-3, the step within 5 % of b's step in norm."""
    num, den = _step_error(sd_a, sd_b, p0)
    print(f"lr {lr_a} / {lr_b}; kls {kls_a} / {kls_b}; step error {num:.3e} of {den:.3e} ({num / den:.4f})")
    assert lr_a == pytest.approx(lr_b, rel=1e-12)
    for a, b in zip(kls_a, kls_b):
        assert a == pytest.approx(b, rel=1e-3)
    assert num <= 0.05 * den, (num, den)


def _torch_update(ex, pol, val, data, perms, epochs, mbs, dtype, device):
    from isaac_rover_orbit_amd.ppo_scaled import TorchScaledPPO
    p, v = ex.Net(2, True), ex.Net(1, False)
    p.load_state_dict(pol.state_dict()); v.load_state_dict(val.state_dict())
    tp = TorchScaledPPO(p.to(dtype), v.to(dtype), epochs=epochs, minibatches=mbs, device=device)
    raw, act, logp, oldv, ret, adv = (x.to(device=device, dtype=dtype) for x in data)
    val_s, ret_s = tp.standardize_values(oldv, ret)
    kls, lr = tp.update(raw, act, logp, val_s, ret_s, adv, perms=[q.to(device) for q in perms])
    return tp, kls, lr


CASES = [(512, 8, 2, 4), (1025, 4, 2, 3)]      # the second: 4100 rows in minibatches of 1367, 1367, 1366, none a multiple of 16


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "-".join(map(str, c)))
def case(request):
    n_env, T, epochs, mbs = request.param
    ex, pol, val = _nets(0)
    data = _inputs(pol, val, T, n_env)
    B = T * n_env
    perms = [torch.randperm(B, device=DEV) for _ in range(epochs)]
    p0 = {r: {k: v.detach().cpu().clone() for k, v in net.state_dict().items()} for r, net in (("policy", pol), ("value", val))}
    return dict(ex=ex, pol=pol, val=val, data=data, perms=perms, p0=p0, epochs=epochs, mbs=mbs, B=B)


def test_the_spec_in_float32_meets_the_bounds_against_its_float64_run(case):
    """On the CPU: the bounds below are ones the reference meets alone on these inputs."""
    c = case
    runs = [_torch_update(c["ex"], c["pol"], c["val"], c["data"], c["perms"], c["epochs"], c["mbs"], dt, "cpu")
            for dt in (torch.float32, torch.float64)]
    (t32, k32, lr32), (t64, k64, lr64) = runs
    _check_bounds(k32, lr32, t32.state_dict(), k64, lr64, t64.state_dict(), c["p0"])


def test_fused_update_tracks_the_torch_spec(case):
    from isaac_rover_orbit_amd.ppo_scaled import FusedScaledPPO
    c = case
    raw, act, logp, oldv, ret, adv = c["data"]
    tp, kls_t, lr_t = _torch_update(c["ex"], c["pol"], c["val"], c["data"], c["perms"], c["epochs"], c["mbs"], torch.float32, DEV)
    tr = FusedScaledPPO(c["pol"].state_dict(), c["val"].state_dict())
    keep = raw.clone()
    val_s, ret_s = tr.standardize_values(oldv, ret)
    kls_f, lr_f = tr.update(raw, act, logp, val_s, ret_s, adv, perms=c["perms"], epochs=c["epochs"], minibatches=c["mbs"])
    assert torch.equal(raw, keep)                                                # the rollout buffer is never written
    _check_bounds(kls_f, lr_f, tr.state_dict(), kls_t, lr_t, tp.state_dict(), c["p0"])
    # both blocks against float64 numpy on the same minibatch order
    ns, nv = NumpyScaler(965), NumpyScaler(1)
    for mb in c["perms"][0].chunk(c["mbs"]):
        ns.train(raw[mb].double().cpu().numpy())
    nv.train(oldv.double().cpu().numpy().reshape(-1, 1))
    nv.train(ret.double().cpu().numpy().reshape(-1, 1))
    sb, vb = tr.state_scaler.block.cpu().numpy(), tr.value_scaler.block.cpu().numpy()
    np.testing.assert_allclose(sb[:965], ns.mean, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(sb[965:1930], ns.var, rtol=1e-12)
    assert sb[1930] == 1 + c["B"] == ns.count                                    # trained in the first epoch only
    np.testing.assert_allclose(vb, [nv.mean[0], nv.var[0], nv.count], rtol=1e-12)
    assert vb[2] == 1 + 2 * c["B"]
    # the image holds the final statistics' rows after the update
    assert _biteq(tr._image[:c["B"]], tr.state_scaler.forward(raw))


def test_identity_scalers_reproduce_the_unscaled_update_bit_for_bit():
    """Initial blocks (mean 0, var 1) and clip = FLT_MAX: forward is x / (1 + 1e-8f) = x in fp32."""
    from isaac_rover_orbit_amd.ppo import FusedPPO
    from isaac_rover_orbit_amd.ppo_scaled import FusedScaledPPO
    ex, pol, val = _nets(0)
    obs, act, logp, oldv, ret, adv = _rollout(pol, val, 4, 512, seed=8, lp_noise=0.15, v_noise=0.3)
    perms = [torch.randperm(2048, device=DEV) for _ in range(2)]
    plain = FusedPPO(pol.state_dict(), val.state_dict())
    out_p = plain.update(obs, act, logp, oldv, ret, adv, perms=perms, epochs=2, minibatches=3)
    tr = FusedScaledPPO(pol.state_dict(), val.state_dict())
    tr.state_scaler.hp.clip = FLT_MAX
    out_s = tr.update(obs, act, logp, oldv, ret, adv, perms=perms, epochs=2, minibatches=3, train_state_scaler=False)
    assert torch.equal(tr.params, plain.params) and out_s == out_p
    assert float(tr.state_scaler.current_count) == 1.0 and _biteq(tr._image[:2048], obs)


def test_checkpoint_round_trip_keeps_the_actor_and_the_blocks(tmp_path):
    from isaac_rover_orbit_amd.ppo_scaled import FusedScaledPPO
    ex, pol, val = _nets(0)
    raw, act, logp, oldv, ret, adv = _inputs(pol, val, 1, 1024, seed=2)
    tr = FusedScaledPPO(pol.state_dict(), val.state_dict())
    val_s, ret_s = tr.standardize_values(oldv, ret)
    tr.update(raw, act, logp, val_s, ret_s, adv, epochs=1, minibatches=2)
    sd = tr.state_dict()
    assert set(sd) == {"policy", "value", "state_preprocessor", "value_preprocessor"}
    path = str(tmp_path / "agent.pt")
    torch.save(sd, path)
    for src in (sd, path):
        back = FusedScaledPPO.from_checkpoint(src)
        assert torch.equal(back.state_scaler.block, tr.state_scaler.block) and torch.equal(back.value_scaler.block, tr.value_scaler.block)
        rows = back.state_scaler.forward(raw[:333].contiguous())
        assert _biteq(rows, tr.state_scaler.forward(raw[:333].contiguous()))
        assert torch.equal(back.actor(rows), tr.actor(rows)) and torch.equal(back.critic(rows), tr.critic(rows))
        assert torch.equal(back.log_std, tr.log_std)
    # a checkpoint without the preprocessor entries loads with the initial blocks
    bare = FusedScaledPPO.from_checkpoint({"policy": sd["policy"], "value": sd["value"]})
    assert float(bare.state_scaler.current_count) == 1.0 and float(bare.value_scaler.current_count) == 1.0
