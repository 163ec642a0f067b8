"""The width-generic running scaler (include/rover_scaler.h) and the rover PPO built on it, without a GPU: sizes against the
Python mirrors, refusals as codes, and the two torch specifications (TorchScaledRollout, TorchScaledPPO) against float64 numpy."""
import ctypes as C

import numpy as np
import pytest
import torch

from lift_ppo_reference import NumpyScaler
from ppo_reference import load_example


def test_sizes_agree_with_the_mirrors():
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    assert lib.rover_scaler_hparams_bytes() == C.sizeof(_lib.ScalerHparams) == 8
    for w in (-1, 0, 1, 2, 63, 64, 65, 965, 1024, 1025, 4096):
        assert lib.rover_scaler_doubles(w) == _lib.scaler_doubles(w) == (2 * w + 1 if 1 <= w <= 1024 else 0), w
        for rows in (-5, 0, 1, 2, 63, 64, 65, 4096, 4099, 245760):
            got = lib.rover_scaler_workspace_bytes(w, rows)
            assert got == _lib.scaler_workspace_bytes(w, rows), (w, rows)
            assert (got > 0) == (1 <= w <= 1024 and rows >= 2)
    # the mean and one float64 partial per column and chunk of 64 rows
    assert lib.rover_scaler_workspace_bytes(965, 4096) == 8 * 965 * (1 + 64)
    assert lib.rover_scaler_workspace_bytes(965, 4097) == 8 * 965 * (1 + 65)
    hp = _lib.ScalerHparams()
    assert lib.rover_scaler_default_hparams(None) == 1
    assert lib.rover_scaler_default_hparams(C.byref(hp)) == 0
    assert hp.eps == np.float32(1e-8) and hp.clip == 5.0


def test_refusals_are_codes_not_crashes():
    """Every invalid argument returns ROVER_ERR_INVALID (1) with a text.  Nothing reaches a GPU: the checks come before any HIP
    call, so the pointers below are never dereferenced."""
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    hp = _lib.ScalerHparams()
    assert lib.rover_scaler_default_hparams(C.byref(hp)) == 0
    BLK, X, OUT, RAW, WS, IDX = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    need = lib.rover_scaler_workspace_bytes(8, 100)

    def train(**kw):
        a = dict(dict(hp=C.byref(hp), blk=BLK, w=8, x=X, idx=None, rows=100, ws=WS, ws_bytes=need), **kw)
        return lib.rover_scaler_train(a["hp"], a["blk"], a["w"], a["x"], a["idx"], a["rows"], a["ws"], a["ws_bytes"], None)

    def apply(**kw):
        a = dict(dict(hp=C.byref(hp), blk=BLK, w=8, x=X, idx=None, rows=100, flags=0, out=OUT, raw=None), **kw)
        return lib.rover_scaler_apply(a["hp"], a["blk"], a["w"], a["x"], a["idx"], a["rows"], a["flags"], a["out"], a["raw"], None)

    for bad, word in ((dict(w=0), b"width"), (dict(w=1025), b"width"), (dict(w=-1), b"width"), (dict(rows=1), b"rows"),
                      (dict(rows=0), b"rows"), (dict(rows=-7), b"rows"), (dict(blk=None), b"NULL"), (dict(hp=None), b"NULL"),
                      (dict(x=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(ws_bytes=need - 8), b"workspace"),
                      (dict(ws_bytes=0), b"workspace"), (dict(blk=BLK + 4), b"aligned"), (dict(idx=IDX + 4), b"aligned"),
                      (dict(x=X + 2), b"aligned")):
        assert train(**bad) == 1, bad
        assert word in lib.rover_last_error(), (bad, lib.rover_last_error())
    # one chunk more than the workspace was sized for
    assert train(rows=129, ws_bytes=lib.rover_scaler_workspace_bytes(8, 128)) == 1
    for bad, word in ((dict(w=0), b"width"), (dict(w=1025), b"width"), (dict(rows=0), b"rows"), (dict(rows=-1), b"rows"),
                      (dict(blk=None), b"NULL"), (dict(hp=None), b"NULL"), (dict(x=None), b"NULL"), (dict(out=None), b"NULL"),
                      (dict(raw=X), b"alias"), (dict(raw=OUT), b"alias"), (dict(raw=X, out=X), b"alias"), (dict(flags=4), b"flag"),
                      (dict(blk=BLK + 4), b"aligned"), (dict(out=OUT + 1), b"aligned"), (dict(raw=RAW + 2), b"aligned")):
        assert apply(**bad) == 1, bad
        assert word in lib.rover_last_error(), (bad, lib.rover_last_error())
    if not torch.cuda.is_available():
        from isaac_rover_orbit_amd.ppo_scaled import FusedScaledPPO
        from isaac_rover_orbit_amd.scaler import DeviceScaler
        # valid arguments, no device: still a code
        assert train() != 0 and apply() != 0 and len(lib.rover_last_error()) > 0
        with pytest.raises(_lib.RoverHipError):
            DeviceScaler(965)                                                  # the product path fails loudly, no CPU fallback
        with pytest.raises(_lib.RoverHipError):
            FusedScaledPPO({}, {})


def _trained_scalers(seed=0):
    from isaac_rover_orbit_amd.lift_ppo import RunningStandardScaler
    g = torch.Generator().manual_seed(seed)
    ss, vs = RunningStandardScaler(965, device="cpu"), RunningStandardScaler(1, device="cpu")
    ss(torch.randn(300, 965, generator=g) * 3.0 + 0.5, train=True)
    vs(torch.randn(300, 1, generator=g) * 7.0 - 2.0, train=True)
    return ss, vs


def test_torch_scaled_rollout_standardises_what_the_networks_see():
    from isaac_rover_orbit_amd import rollout as R
    from isaac_rover_orbit_amd.rollout_scaled import TorchScaledRollout
    n, T = 23, 2
    ss, vs = _trained_scalers()
    seen = []
    w = torch.linspace(-1, 1, 965)

    def actor(s):
        seen.append(s.clone())
        return torch.tanh(s[:, :2] * 0.3)

    def critic(s):
        seen.append(s.clone())
        return (s * w).sum(1, keepdim=True) * 0.05

    g = torch.Generator().manual_seed(3)
    raw = torch.randn(n, 965, generator=g) * 4.0
    raw[0, 5], raw[1, 6], raw[2, 964], raw[3, 100] = float("-inf"), float("nan"), float("inf"), 1e6
    log_std = torch.tensor([-0.3, 0.2])
    ro = TorchScaledRollout(actor, critic, log_std, ss, vs, n, T, seed=9, device="cpu")
    plain = R.TorchRollout(lambda o: actor(ss(o)), lambda o: critic(ss(o)), log_std, n, T, seed=9, device="cpu")
    ea = ro.act(0, raw)
    san = R.TorchRollout.sanitise(raw)
    assert torch.equal(ro.obs[0], san) and torch.isfinite(ro.obs[0]).all()
    assert len(seen) == 2 and all(torch.equal(s, ss(san)) for s in seen)
    assert float(seen[0].abs().max()) == 5.0                                   # the clamp is part of what they see
    v_s = critic(ss(san))
    assert torch.equal(ro.val[0], vs(v_s, inverse=True).reshape(n))
    assert torch.equal(ro.val[0], (torch.sqrt(vs.running_variance.float()) * v_s.clamp(-5, 5) + vs.running_mean.float()).reshape(n))
    # the draws, actions and log-probabilities are TorchRollout's on the standardised rows
    eb = plain.act(0, raw)
    assert torch.equal(ea, eb) and torch.equal(ro.actions[0], plain.actions[0]) and torch.equal(ro.logp[0], plain.logp[0])
    assert torch.equal(ro.mean[0], plain.mean[0]) and ro.counter == 1
    assert torch.equal(ro.last_value(raw), ro.val[0]) and ro.counter == 1
    # by reference: a scaler update between two steps is seen
    old = ss(san)
    ss(torch.randn(50, 965, generator=g) + 3.0, train=True)
    seen.clear()
    ro.act(1, raw)
    assert torch.equal(seen[0], ss(san)) and not torch.equal(seen[0], old)
    assert ro.state_dict() == {"seed": 9, "counter": 2, "env_id_offset": 0}


def _cpu_rollout(ex, B, seed=1):
    g = torch.Generator().manual_seed(seed)
    col = torch.rand(965, generator=g)
    obs = torch.randn(B, 965, generator=g) * (0.2 + 4.0 * col) + (col - 0.5) * 6.0
    act = torch.randn(B, 2, generator=g)
    logp = torch.randn(B, generator=g) * 0.3 - 2.0
    val, ret, adv = (torch.randn(B, generator=g) for _ in range(3))
    return obs, act, logp, val, ret, adv


def test_torch_scaled_ppo_trains_the_state_scaler_in_the_first_epoch_only():
    from isaac_rover_orbit_amd.ppo_scaled import TorchScaledPPO
    ex = load_example()
    torch.manual_seed(0)
    B, E, M = 97, 3, 4
    tp = TorchScaledPPO(ex.Net(2, True), ex.Net(1, False), epochs=E, minibatches=M, device="cpu")
    obs, act, logp, val, ret, adv = _cpu_rollout(ex, B)
    g = torch.Generator().manual_seed(5)
    perms = [torch.randperm(B, generator=g) for _ in range(E)]
    ns, nv = NumpyScaler(965), NumpyScaler(1)
    nv.train(val.double().numpy().reshape(-1, 1))
    v_expect = nv.forward(val.double().numpy().reshape(-1, 1))
    nv.train(ret.double().numpy().reshape(-1, 1))
    r_expect = nv.forward(ret.double().numpy().reshape(-1, 1))
    val_s, ret_s = tp.standardize_values(val, ret)
    assert float(tp.value_preprocessor.current_count) == 1 + 2 * B
    np.testing.assert_allclose(val_s.numpy(), v_expect[:, 0], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(ret_s.numpy(), r_expect[:, 0], rtol=1e-4, atol=1e-5)
    p0 = [p.detach().clone() for p in tp.policy.parameters()]
    kls, lr = tp.update(obs, act, logp, val_s, ret_s, adv, perms=perms)
    assert len(kls) == E and all(np.isfinite(kls)) and lr == tp.lr
    assert any(not torch.equal(a, b) for a, b in zip(p0, tp.policy.parameters()))
    for mb in perms[0].chunk(M):
        ns.train(obs[mb].double().numpy())
    assert float(tp.state_preprocessor.current_count) == 1 + B == ns.count
    np.testing.assert_allclose(tp.state_preprocessor.running_mean.numpy(), ns.mean, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(tp.state_preprocessor.running_variance.numpy(), ns.var, rtol=1e-4)
    np.testing.assert_allclose(tp.value_preprocessor.running_mean.numpy(), nv.mean, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(tp.value_preprocessor.running_variance.numpy(), nv.var, rtol=1e-4)
    # a frozen scaler stays where it is
    before = tp.state_preprocessor.state_dict()
    tp.update(obs, act, logp, val_s, ret_s, adv, perms=perms, epochs=1, train_state_scaler=False)
    assert all(torch.equal(before[k], v) for k, v in tp.state_preprocessor.state_dict().items())


def test_checkpoint_keys_round_trip():
    from isaac_rover_orbit_amd.lift_ppo import RunningStandardScaler
    from isaac_rover_orbit_amd.ppo_scaled import TorchScaledPPO
    ex = load_example()
    torch.manual_seed(1)
    tp = TorchScaledPPO(ex.Net(2, True), ex.Net(1, False), device="cpu")
    tp.state_preprocessor, tp.value_preprocessor = _trained_scalers(4)
    sd = tp.state_dict()
    assert set(sd) == {"policy", "value", "state_preprocessor", "value_preprocessor"}
    for key, w in (("state_preprocessor", 965), ("value_preprocessor", 1)):
        assert set(sd[key]) == {"running_mean", "running_variance", "current_count"}
        assert sd[key]["running_mean"].shape == (w,) and sd[key]["running_mean"].dtype == torch.float64
        back = RunningStandardScaler(w, device="cpu")
        back.load_state_dict(sd[key])
        assert all(torch.equal(v, back.state_dict()[k]) for k, v in sd[key].items())
        assert float(back.current_count) == 301.0
    net = ex.Net(2, True)
    net.load_state_dict(sd["policy"])


# ------------------------------------------------------------------------------------- the documented order and the fp32 oracle
def test_ordered_train_is_numpy_scaler_within_the_existing_bound():
    """The restated reduction order computes what NumpyScaler does, at tests/test_gpu_scaler.py's bounds and on its kind of data."""
    import scaler_cases as SC
    g = np.random.default_rng(0)
    for w, rows in ((1, 2), (3, 63), (65, 64), (5, 65), (129, 257), (2, 4099)):
        ns, blk = NumpyScaler(w), SC.initial_block(w)
        for i in range(4):
            x = (g.standard_normal((rows, w)) * (1 + 3 * i) + i).astype(np.float32)
            ns.train(x.astype(np.float64))
            blk = SC.ordered_train(blk, x)
            np.testing.assert_allclose(blk[:w], ns.mean, rtol=1e-12, atol=1e-12, err_msg=f"mean w={w} rows={rows} call={i}")
            np.testing.assert_allclose(blk[w:2 * w], ns.var, rtol=1e-12, err_msg=f"var w={w} rows={rows} call={i}")
            assert blk[2 * w] == ns.count == 1 + (i + 1) * rows


def test_ordered_train_on_hard_columns_against_exact_arithmetic():
    """What the documented order can deliver on columns with |mean| / sd up to 1e8 (profiles/scaler_edges_margins.txt has the
    figures): per column the relative error of the merged mean and variance against exact rational arithmetic stays below
    HARD_BOUND_CONSTANT * (|offset| / sd + 1) * 2**-52; a constant column's batch variance stays below (rows * 2**-52 * |c|)**2."""
    import scaler_cases as SC
    worst = SC.hard_margins()
    print(SC.margins_text())
    for c, (name, (m, v, ratio)) in enumerate(zip(SC.HARD_NAMES, worst)):
        if c in SC.HARD_CONSTANT:
            assert ratio <= 1.0, (name, ratio)
            assert m <= 1027 * SC.U, (name, m)                                 # a sum of `rows` equal terms, then the merge
        else:
            assert ratio <= SC.HARD_BOUND_CONSTANT, (name, m, v, ratio)
    # rtol 1e-12 is not a bound the documented order meets here: the tests of the device hold it to the order's own bits instead
    assert max(v for _, v, _ in worst) > 1e-12


@pytest.mark.parametrize("w", [12, 65, 257])
def test_the_two_fp32_oracles_agree_bit_for_bit_on_edge_blocks(w):
    """torch on CPU tensors and numpy float32 give the same bits (NaN matching NaN) for forward, inverse and the sanitised forms on
    blocks whose (float)var is 0, subnormal, FLT_MAX or inf: either is the CPU oracle of the device tests."""
    import scaler_cases as SC
    blk, x = SC.edge_block(w), SC.edge_rows(w)
    assert x.shape == (17, w) and np.isnan(x).any() and np.isinf(x).any()
    tb, tx = torch.from_numpy(blk), torch.from_numpy(x)
    assert SC.same_bits32(SC.torch_sanitise(tx).numpy(), SC.numpy_sanitise(x))
    for eps, clip in SC.HPARAMS:
        for rows_t, rows_n in ((tx, x), (SC.torch_sanitise(tx), SC.numpy_sanitise(x))):
            f_t, f_n = SC.torch_forward(rows_t, tb, w, eps, clip).numpy(), SC.numpy_forward(rows_n, blk, w, eps, clip)
            i_t, i_n = SC.torch_inverse(rows_t, tb, w, clip).numpy(), SC.numpy_inverse(rows_n, blk, w, clip)
            assert f_t.dtype == f_n.dtype == i_t.dtype == i_n.dtype == np.float32
            assert SC.same_bits32(f_t, f_n), (eps, clip)
            assert SC.same_bits32(i_t, i_n), (eps, clip)
    # the hard cells are there: a zero, a subnormal, the largest and an infinite (float)var, NaN from 0 / 0 and inf / inf
    f = SC.numpy_forward(x, blk, w, 0.0, 5.0)
    with np.errstate(over="ignore"):
        var32 = blk[w:2 * w].astype(np.float32)
    assert (var32 == 0).any() and ((var32 > 0) & (var32 < SC.FLT_MIN)).any() and np.isinf(var32).any() and (var32 == SC.FLT_MAX).any()
    assert np.isnan(f[0]).any() and (np.abs(f[~np.isnan(f)]) <= 5.0).all()
