"""Fused PPO update, CPU side: the packed layout round-trips through rover_policy_unpack, and the float64 reference of the
update (tests/ppo_reference.py) is pinned to examples/04_train_ppo.py's own loss."""
import ctypes as C

import numpy as np
import pytest
import torch

from ppo_reference import load_example, loss_and_grads


def _random_sd(out_dim, final_tanh, seed):
    ex = load_example()
    torch.manual_seed(seed)
    net = ex.Net(out_dim, final_tanh)
    if final_tanh:
        with torch.no_grad():
            net.log_std_parameter.copy_(torch.tensor([-0.4, 0.3]))
    return net


@pytest.mark.parametrize("out_dim,final_act", [(2, "tanh"), (1, "none")])
def test_unpack_inverts_pack_and_padding_is_zero(out_dim, final_act):
    from isaac_rover_orbit_amd import _lib, build
    from isaac_rover_orbit_amd.ppo import pack, unpack
    build.build_extension()
    sd = _random_sd(out_dim, final_act == "tanh", 3).state_dict()
    desc, packed = pack(sd, final_act)
    back = unpack(desc, packed)
    for k, v in back.items():
        assert torch.equal(v, sd[k]), k
    # every float of the packed buffer that is no weight or bias is exactly 0
    used = np.zeros(packed.size, bool)
    for i in range(desc.n_enc + desc.n_mlp):
        L = desc.layers[i]
        G = (L.K + 15) // 16
        n, k = np.meshgrid(np.arange(L.N), np.arange(L.K), indexing="ij")
        pos = L.w_off + ((((n >> 4) * G + (k >> 4)) * 64 + (n & 15) + 16 * (k & 3)) << 2) + ((k >> 2) & 3)
        used[pos.ravel()] = True
        used[L.b_off:L.b_off + L.N] = True
    assert used.sum() == sum(v.numel() for k, v in sd.items() if k != "log_std_parameter")
    assert np.all(packed[~used] == 0.0)
    lib = _lib.load()
    assert lib.rover_policy_unpack(None, None, None, None) == 1


def test_param_floats_and_refusals_on_the_host():
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd.ppo import default_hparams, pack
    lib = _lib.load()
    dp, pa = pack(_random_sd(2, True, 1).state_dict(), "tanh")
    dv, pv = pack(_random_sd(1, False, 2).state_dict(), "none")
    assert lib.rover_ppo_param_floats(C.byref(dp), C.byref(dv)) == pa.size + pv.size + 4
    assert lib.rover_ppo_param_floats(C.byref(dv), C.byref(dp)) == 0          # roles swapped: not the reference pair
    assert lib.rover_ppo_workspace_bytes(0) == 0 and lib.rover_ppo_workspace_bytes(16) > 0
    h = default_hparams()
    assert (h.gamma, h.lam, h.clip_ratio, h.value_clip, h.max_grad_norm) == pytest.approx((0.99, 0.95, 0.2, 0.2, 0.5))
    bad = _lib.PolicyDesc.from_buffer_copy(dp)
    bad.layers[2].N = 128
    args = [None] * 8 + [0, None, 0] + [None] * 5      # params .. adv, idx; n = 0; ws, bytes = 0; grad, stats, outs, stream
    assert lib.rover_ppo_minibatch(C.byref(bad), C.byref(dv), C.byref(h), *args) == 4     # ROVER_ERR_UNSUPPORTED
    assert lib.rover_ppo_minibatch(C.byref(dp), C.byref(dv), C.byref(h), *args) == 1      # NULL buffers: ROVER_ERR_INVALID


def test_float64_reference_matches_the_example_loss():
    """On one CPU minibatch the float64 restatement and the example's ppo_loss (fp32 autograd) agree on loss, KL and every
    gradient, with ratios on both sides of the clip and the value clip active."""
    ex = load_example()
    pol, val = _random_sd(2, True, 11), _random_sd(1, False, 12)
    g = torch.Generator().manual_seed(5)
    n = 256
    o = torch.randn(n, 965, generator=g) * 0.5
    with torch.no_grad():
        mean = pol(o)
        v0 = val(o)[:, 0]
    a = mean + 0.7 * torch.randn(n, 2, generator=g)
    ls = pol.log_std_parameter.detach()
    lp = (-0.5 * ((a - mean) / ls.exp()) ** 2 - ls - 0.9189385332).sum(1)
    old_lp = lp + 0.3 * torch.randn(n, generator=g)
    old_v = v0 + 0.4 * torch.randn(n, generator=g)
    ret = old_v + torch.randn(n, generator=g)
    adv = torch.randn(n, generator=g)
    loss32, kl32 = ex.ppo_loss(pol, val, o, a, old_lp, old_v, ret, adv)
    loss32.backward()
    loss64, kl64, g64 = loss_and_grads(pol.state_dict(), val.state_dict(), o, a, old_lp, old_v, ret, adv)
    assert float(loss32.detach()) == pytest.approx(float(loss64), rel=1e-5)
    assert float(kl32) == pytest.approx(float(kl64), rel=1e-4)
    for role, net in (("policy", pol), ("value", val)):
        for k, p in net.named_parameters():
            ref = g64[role][k]
            err = float((p.grad.double() - ref).norm())
            assert err <= 1e-4 * float(ref.norm()) + 1e-9, (role, k, err)
