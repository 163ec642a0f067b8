"""Fused TRPO, CPU side: the torch spec's double-backward Fisher-vector product is the Gauss-Newton product the kernels
implement, CG follows skrl's residual rule, a rejected line search restores the policy bit for bit, the cumulative expected
improvement decides as skrl's loop does, and the host-only parts of include/rover_trpo.h."""
import ctypes as C

import numpy as np
import pytest
import torch

from ppo_reference import load_example


def _policy(seed=0, log_std=(-0.4, 0.3), dtype=torch.float64):
    ex = load_example()
    torch.manual_seed(seed)
    pol = ex.Net(2, True).to(dtype)
    with torch.no_grad():
        pol.log_std_parameter.copy_(torch.tensor(log_std, dtype=dtype))
    return pol


@pytest.mark.parametrize("log_std", [(-0.4, 0.3), (-21.0, 2.5), (1.0, -25.0)])
def test_double_backward_fvp_is_gauss_newton(log_std):
    from isaac_rover_orbit_amd.trpo import fisher_vector_product, gauss_newton_fvp
    pol = _policy(1, log_std)
    g = torch.Generator().manual_seed(2)
    obs = torch.randn(48, 965, dtype=torch.float64, generator=g) * 0.5
    n = sum(p.numel() for p in pol.parameters())
    for _ in range(2):
        v = torch.randn(n, dtype=torch.float64, generator=g)
        a = fisher_vector_product(pol, obs, v, damping=0.1)
        b = gauss_newton_fvp(pol, obs, v, damping=0.1)
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-10 * float(b.abs().max())), float((a - b).abs().max())


def test_conjugate_gradient_meets_skrl_residual_rule():
    from isaac_rover_orbit_amd.trpo import conjugate_gradient
    g = torch.Generator().manual_seed(0)
    M = torch.randn(6, 6, dtype=torch.float64, generator=g)
    A = M @ M.T + 0.5 * torch.eye(6, dtype=torch.float64)
    b = torch.randn(6, dtype=torch.float64, generator=g)
    x, it, rr = conjugate_gradient(lambda p: A @ p, b, num_iterations=10, residual_tolerance=1e-10)
    # exact arithmetic ends a 6-dimensional problem within 6 iterations: the loop stops at the first r.r below the tolerance
    assert it <= 7 and rr < 1e-10
    assert torch.allclose(A @ x, b, atol=1e-5)
    # and with too few iterations it runs all of them and reports the unconverged residual r = b - A x
    x2, it2, rr2 = conjugate_gradient(lambda p: A @ p, b, num_iterations=2, residual_tolerance=1e-10)
    assert it2 == 2 and rr2 > 1e-10
    assert abs(rr2 - float(((b - A @ x2) ** 2).sum())) < 1e-8 * max(rr2, 1.0)


def test_cumulative_expected_improvement_decides_like_skrl():
    from isaac_rover_orbit_amd.trpo import line_search
    # improvement of trial i = 0.3 x 0.5^i: against alpha_i E it is always 0.3 (never accepted), against skrl's cumulative
    # product E prod_{j<=i} alpha_j it is 0.3 x 2^(i (i - 1) / 2): 0.3, 0.3, 0.6 -> trial 2
    theta = torch.zeros(3)
    full = torch.ones(3)
    evaluate = lambda th: (0.0, 0.3 * float(th[0]))  # noqa: E731
    acc, th, _, _ = line_search(theta, full, 1.0, evaluate, 0.0, max_kl=0.01, accept_ratio=0.5)
    assert acc == 2 and torch.equal(th, 0.25 * full)
    acc, th, _, _ = line_search(theta, full, 1.0, lambda t: (1.0, 1.0), 0.0, max_kl=0.01, accept_ratio=0.5)
    assert acc == -1 and th is theta


def test_rejected_line_search_restores_policy_bit_for_bit():
    from isaac_rover_orbit_amd.trpo import TorchTRPO
    ex = load_example()
    torch.manual_seed(3)
    pol, val = ex.Net(2, True), ex.Net(1, False)
    g = torch.Generator().manual_seed(4)
    B = 64
    obs = torch.randn(B, 965, generator=g) * 0.5
    with torch.no_grad():
        mean = pol(obs)
        act = mean + torch.randn(B, 2, generator=g)
        logp = (-0.5 * (act - mean) ** 2 - 0.9189385332).sum(1) + 0.1 * torch.randn(B, generator=g)
    adv = torch.randn(B, generator=g)
    before = [p.detach().clone() for p in pol.parameters()]
    st = TorchTRPO(pol, val, max_kl_divergence=1e-30).policy_step(obs, act, logp, adv)
    assert st["accepted"] == -1
    for p, b in zip(pol.parameters(), before):
        assert torch.equal(p, b)
    st = TorchTRPO(pol, val).policy_step(obs, act, logp, adv)
    assert st["accepted"] >= 0 and st["kl"] < 0.01
    assert any(not torch.equal(p, b) for p, b in zip(pol.parameters(), before))


# ---- host-only ABI checks
def _descs():
    from isaac_rover_orbit_amd.ppo import pack
    ex = load_example()
    torch.manual_seed(0)
    dp, _ = pack(ex.Net(2, True).state_dict(), "tanh")
    dv, _ = pack(ex.Net(1, False).state_dict(), "none")
    return dp, dv


def test_default_hparams_match_the_spec():
    from isaac_rover_orbit_amd import build
    from isaac_rover_orbit_amd.trpo import HPARAMS, default_hparams
    build.build_extension()
    h = default_hparams()
    want = dict(gamma=HPARAMS["discount_factor"], lam=HPARAMS["lambda_"], value_loss_scale=HPARAMS["value_loss_scale"],
                log_std_min=HPARAMS["log_std_min"], log_std_max=HPARAMS["log_std_max"], max_grad_norm=HPARAMS["grad_norm_clip"],
                beta1=0.9, beta2=0.999, eps=1e-8, value_lr=HPARAMS["value_learning_rate"], damping=HPARAMS["damping"],
                max_kl=HPARAMS["max_kl_divergence"], cg_tol=HPARAMS["cg_residual_tolerance"], accept_ratio=HPARAMS["accept_ratio"],
                step_fraction=HPARAMS["step_fraction"], cg_steps=HPARAMS["conjugate_gradient_steps"],
                max_backtrack=HPARAMS["max_backtrack_steps"])
    for k, v in want.items():
        assert getattr(h, k) == pytest.approx(v, rel=1e-7), k
    assert HPARAMS["learning_rate"] == 1e-4 and HPARAMS["value_learning_rate"] == 1e-3


def test_struct_param_and_workspace_sizes():
    from isaac_rover_orbit_amd import _lib, build
    build.build_extension()
    lib = _lib.load()
    assert lib.rover_trpo_hparams_bytes() == C.sizeof(_lib.TrpoHparams) == 68
    assert lib.rover_trpo_state_bytes() == C.sizeof(_lib.TrpoState) == 96
    dp, dv = _descs()
    P = lib.rover_trpo_param_floats(C.byref(dp), C.byref(dv))
    assert P == lib.rover_ppo_param_floats(C.byref(dp), C.byref(dv)) == lib.rover_policy_packed_floats(C.byref(dp)) + \
        lib.rover_policy_packed_floats(C.byref(dv)) + 4
    assert lib.rover_trpo_param_floats(C.byref(dv), C.byref(dp)) == 0
    # 1024 head floats, 7 vectors of P (padded to 4), per network region 2 x 690 floats per row, row partials and the 2048-row
    # chunk partials of the weight gradients
    Pp, Pv = lib.rover_policy_packed_floats(C.byref(dp)), lib.rover_policy_packed_floats(C.byref(dv))

    def region(rows, pn):
        return 2 * 690 * rows + ((4 * -(-rows // 256) + 3) & ~3) + -(-rows // 2048) * pn
    for B, mb in ((1, 1), (256, 17), (60 * 4096, 4096)):
        want = 4 * (1024 + 7 * ((P + 3) & ~3) + region(B, Pp) + region(mb, Pv))
        assert lib.rover_trpo_workspace_bytes(B, mb) == want
    assert lib.rover_trpo_workspace_bytes(0, 1) == 0 and lib.rover_trpo_workspace_bytes(1, 0) == 0


def test_non_reference_descriptor_is_unsupported():
    from isaac_rover_orbit_amd import _lib, build
    from isaac_rover_orbit_amd.trpo import default_hparams
    build.build_extension()
    lib = _lib.load()
    dp, dv = _descs()
    h = default_hparams()
    bad = _lib.PolicyDesc.from_buffer_copy(dp)
    bad.layers[2].N = 255
    assert lib.rover_trpo_policy_grad(C.byref(bad), C.byref(dv), C.byref(h), None, None, None, None, None, 1, None, 0, None, None,
                                      None) == 4
    assert b"reference architecture" in lib.rover_last_error()
    assert lib.rover_trpo_fvp(C.byref(dp), C.byref(bad), C.byref(h), None, None, 1, None, 0, None, None, None) == 4
    assert lib.rover_trpo_policy_step(C.byref(bad), C.byref(dv), C.byref(h), None, None, None, None, None, 1, None, 0, None, None, 1,
                                      None, None, None) == 4
    assert lib.rover_trpo_value_minibatch(C.byref(dp), C.byref(bad), C.byref(h), None, None, None, None, 1, 1, None, 0, None, None,
                                          None) == 4
    assert lib.rover_trpo_value_apply(C.byref(bad), C.byref(dv), C.byref(h), None, None, None, None, None, None, 1, None, 0, None) == 4
