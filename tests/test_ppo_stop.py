"""skrl's KL early stop, scheduler switch and reward shaping for the rover PPO, without a GPU: the new structs against their
mirrors, refusals as codes, the torch specification (ppo_skrl.TorchSkrlPPO, shape_rewards) against the updates it generalises,
and the example's flags."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

from ppo_reference import load_example


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_struct_sizes_agree_with_the_mirrors_and_the_old_ones_have_not_moved():
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    assert lib.rover_ppo_epoch_bytes() == C.sizeof(_lib.PpoEpoch) == 32
    offs = {n: getattr(_lib.PpoEpoch, n).offset for n, _ in _lib.PpoEpoch._fields_}
    assert offs == {"stop": 0, "recorded": 4, "epochs": 8, "stopped_epochs": 12, "stop_minibatch": 16, "stop_kl": 20, "reserved": 24}
    assert lib.rover_ppo_hparams_bytes() == C.sizeof(_lib.PpoHparams) == 60
    assert lib.rover_ppo_state_bytes() == C.sizeof(_lib.PpoState) == 32
    assert lib.rover_scaler_hparams_bytes() == C.sizeof(_lib.ScalerHparams) == 8
    assert lib.rover_rollout_hparams_bytes() == C.sizeof(_lib.RolloutHparams) == 32
    for name in ("rover_ppo_minibatch_gated", "rover_ppo_apply_gated", "rover_ppo_epoch_end", "rover_scaler_train_gated",
                 "rover_rollout_record_shaped"):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def _descs():
    from isaac_rover_orbit_amd.ppo import default_hparams, pack
    ex = load_example()
    torch.manual_seed(3)
    dp, _ = pack(ex.Net(2, True).state_dict(), "tanh")
    dv, _ = pack(ex.Net(1, False).state_dict(), "none")
    return dp, dv, default_hparams()


def test_refusals_of_the_gated_entries_are_codes():
    """ROVER_ERR_INVALID (1) with a text, before any HIP call: the made-up pointers are never dereferenced."""
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    dp, dv, h = _descs()
    P, G, WS, EP, ST = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    need = lib.rover_ppo_workspace_bytes(64)

    def mb(**kw):
        a = dict(dict(h=C.byref(h), params=P, obs=P, act=P, logp=P, val=P, ret=P, adv=P, idx=P, n=64, ws=WS, ws_bytes=need, grad=G,
                      stats=G, thr=0.008, ep=EP), **kw)
        return lib.rover_ppo_minibatch_gated(C.byref(dp), C.byref(dv), a["h"], a["params"], a["obs"], a["act"], a["logp"], a["val"],
                                             a["ret"], a["adv"], a["idx"], a["n"], a["ws"], a["ws_bytes"], a["grad"], a["stats"], None,
                                             None, a["thr"], a["ep"], None)

    def ap(**kw):
        a = dict(dict(h=C.byref(h), params=P, grad=G, m=G, v=G, st=ST, ws=WS, ws_bytes=need, ep=EP, copies=1), **kw)
        return lib.rover_ppo_apply_gated(C.byref(dp), C.byref(dv), a["h"], a["params"], a["grad"], a["m"], a["v"], a["st"], None, None,
                                         a["copies"], a["ws"], a["ws_bytes"], a["ep"], None)

    def end(**kw):
        a = dict(dict(h=C.byref(h), stats=G, n=4, st=ST, ep=EP, sched=0), **kw)
        return lib.rover_ppo_epoch_end(a["h"], a["stats"], a["n"], a["st"], a["ep"], a["sched"], None, None)

    for fn, cases in ((mb, ((dict(ep=None), b"NULL"), (dict(ep=EP + 4), b"aligned"), (dict(h=None), b"NULL"), (dict(idx=None), b"NULL"),
                            (dict(stats=None), b"NULL"), (dict(n=0), b"n must"), (dict(n=-3), b"n must"),
                            (dict(ws_bytes=need - 4), b"workspace"), (dict(ws=WS + 8), b"aligned"))),
                      (ap, ((dict(ep=None), b"NULL"), (dict(ep=EP + 4), b"aligned"), (dict(h=None), b"NULL"), (dict(st=None), b"NULL"),
                            (dict(st=ST + 4), b"aligned"), (dict(ws_bytes=0), b"workspace"))),
                      (end, ((dict(ep=None), b"NULL"), (dict(ep=EP + 4), b"aligned"), (dict(st=ST + 4), b"aligned"),
                             (dict(stats=None), b"NULL"), (dict(h=None), b"NULL"), (dict(n=0), b"n_minibatches"),
                             (dict(n=-1), b"n_minibatches"), (dict(sched=2), b"schedule")))):
        for bad, word in cases:
            assert fn(**bad) == 1, (fn.__name__, bad)
            assert word in lib.rover_last_error(), (bad, lib.rover_last_error())
    bad = _lib.PolicyDesc.from_buffer_copy(dp)
    bad.layers[2].N = 128
    assert lib.rover_ppo_minibatch_gated(C.byref(bad), C.byref(dv), C.byref(h), *([P] * 8), 64, WS, need, G, G, None, None, 0.008, EP,
                                         None) == 4                                        # ROVER_ERR_UNSUPPORTED

    hp = _lib.ScalerHparams()
    assert lib.rover_scaler_default_hparams(C.byref(hp)) == 0
    sneed = lib.rover_scaler_workspace_bytes(8, 100)

    def train(**kw):
        a = dict(dict(hp=C.byref(hp), blk=P, w=8, x=G, idx=None, rows=100, ws=WS, ws_bytes=sneed, gate=EP), **kw)
        return lib.rover_scaler_train_gated(a["hp"], a["blk"], a["w"], a["x"], a["idx"], a["rows"], a["ws"], a["ws_bytes"], a["gate"], None)

    for bad, word in ((dict(gate=None), b"NULL"), (dict(gate=EP + 2), b"aligned"), (dict(hp=None), b"NULL"), (dict(blk=None), b"NULL"),
                      (dict(rows=1), b"rows"), (dict(rows=0), b"rows"), (dict(w=1025), b"width"), (dict(ws_bytes=sneed - 8), b"workspace"),
                      (dict(blk=P + 4), b"aligned")):
        assert train(**bad) == 1, bad
        assert word in lib.rover_last_error(), (bad, lib.rover_last_error())

    def rec(**kw):
        a = dict(dict(rew=P, term=P, trunc=P, val=P, n=8, boot=1, ro=G, do=G), **kw)
        return lib.rover_rollout_record_shaped(a["rew"], a["term"], a["trunc"], a["val"], a["n"], 0.5, 0.99, a["boot"], a["ro"], a["do"],
                                               None)

    for bad, word in ((dict(rew=None), b"NULL"), (dict(term=None), b"NULL"), (dict(trunc=None), b"NULL"), (dict(ro=None), b"NULL"),
                      (dict(do=None), b"NULL"), (dict(val=None), b"val is NULL"), (dict(n=0), b"n must"), (dict(n=-2), b"n must"),
                      (dict(ro=G + 2), b"aligned"), (dict(val=P + 1), b"aligned")):
        assert rec(**bad) == 1, bad
        assert word in lib.rover_last_error(), (bad, lib.rover_last_error())
    if not torch.cuda.is_available():
        # valid arguments, no device: still a code
        assert ap() != 0 and end() != 0 and train() != 0 and len(lib.rover_last_error()) > 0


# ------------------------------------------------------------------------------------------------------------------ the spec
def _cpu_rollout(pol, val, B, seed=1, dtype=torch.float32, noise=0.05):
    """Rows with per-column scales and offsets; old log-probabilities and values close to the networks' own on the rows a fresh
    state scaler first shows them, so that the KL starts small and climbs with the steps."""
    from isaac_rover_orbit_amd.trpo import log_prob
    g = torch.Generator().manual_seed(seed)
    col = torch.rand(965, generator=g)
    rn = lambda *shape: torch.randn(*shape, generator=g).to(dtype)  # noqa: E731
    obs = rn(B, 965) * (0.2 + 4.0 * col).to(dtype) + ((col - 0.5) * 6.0).to(dtype)
    s = ((obs - obs.mean(0)) / obs.std(0)).clamp(-5, 5)
    with torch.no_grad():
        mean = pol(s)
        act = mean + pol.log_std_parameter.exp() * rn(B, 2)
        logp = log_prob(pol, s, act) + noise * rn(B)
        v = val(s)[:, 0] + 0.1 * rn(B)
    ret = v + 0.3 * rn(B)
    adv = rn(B)
    return obs, act, logp, v, ret, adv


def _pair(ex, seed=0, dtype=torch.float32):
    torch.manual_seed(seed)
    return ex.Net(2, True).to(dtype), ex.Net(1, False).to(dtype)


def _clone(ex, nets, dtype=torch.float32):
    out = (ex.Net(2, True).to(dtype), ex.Net(1, False).to(dtype))
    for a, b in zip(out, nets):
        a.load_state_dict(b.state_dict())
    return out


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.parameters(), b.parameters()))


def _perms(B, E, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(B, generator=g) for _ in range(E)]


def test_stop_off_and_kl_adaptive_is_torch_scaled_ppo():
    from isaac_rover_orbit_amd.ppo_scaled import TorchScaledPPO
    from isaac_rover_orbit_amd.ppo_skrl import TorchSkrlPPO
    ex = load_example()
    B, E, M = 97, 3, 4
    nets = _pair(ex)
    data, perms = _cpu_rollout(*nets, B), _perms(B, E)
    a = TorchScaledPPO(*_clone(ex, nets), lr=3e-3, epochs=E, minibatches=M, device="cpu")
    b = TorchSkrlPPO(*_clone(ex, nets), lr=3e-3, epochs=E, minibatches=M, device="cpu")
    outs = []
    for t in (a, b):
        obs, act, logp, v, ret, adv = data
        vs, rs = t.standardize_values(v, ret)
        outs.append(t.update(obs, act, logp, vs, rs, adv, perms=perms))
    assert outs[0] == outs[1] and a.lr != 3e-3                                         # the scheduler moved the rate, identically
    assert _same(a.policy, b.policy) and _same(a.value, b.value)
    for k in ("state_preprocessor", "value_preprocessor"):
        assert all(torch.equal(v, b.state_dict()[k][n]) for n, v in a.state_dict()[k].items())
    assert b.last_update == {"recorded": [M] * E, "stopped": [False] * E} and b.steps == E * M


def test_without_scalers_it_is_the_examples_update_step_for_step_in_float64():
    """examples/04_train_ppo.py's torch update (its loop restated around its own ppo_loss), compared after every epoch."""
    from isaac_rover_orbit_amd.ppo_skrl import TorchSkrlPPO
    ex = load_example()
    B, E, M, dt = 61, 3, 3, torch.float64
    nets = _pair(ex, 1, dt)
    obs, act, logp, v, ret, adv = _cpu_rollout(*nets, B, seed=2, dtype=dt)
    s = ((obs - obs.mean(0)) / obs.std(0)).clamp(-5, 5)                                 # the rows the old log-probabilities were taken on
    perms = _perms(B, E)
    pol, val = _clone(ex, nets, dt)
    params = list(pol.parameters()) + list(val.parameters())
    opt = torch.optim.Adam(params, lr=2e-3)
    t = TorchSkrlPPO(*_clone(ex, nets, dt), lr=2e-3, epochs=E, minibatches=M, scalers=False, device="cpu")
    assert t.standardize_values(v, ret) == (v, ret)
    for e in range(E):
        kls = []
        for mb in perms[e].chunk(M):                                                    # examples/04_train_ppo.py, the torch update
            loss, kl = ex.ppo_loss(pol, val, s[mb], act[mb], logp[mb], v[mb], ret[mb], adv[mb], ex.CLIP, ex.VCLIP)
            kls.append(kl)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            nn.utils.clip_grad_norm_(params, 0.5)
            opt.step()
        kl_mean = torch.stack(kls).mean().item()
        lr = opt.param_groups[0]["lr"]
        if kl_mean > 2 * ex.KL_THR: lr = max(lr / 1.5, 1e-6)
        elif kl_mean < 0.5 * ex.KL_THR: lr = min(lr * 1.5, 1e-2)
        for g in opt.param_groups: g["lr"] = lr
        got, lr_t = t.update(s, act, logp, v, ret, adv, perms=[perms[e]], epochs=1)
        assert got == [kl_mean] and lr_t == lr, e
        assert _same(pol, t.policy) and _same(val, t.value), e
    assert set(t.state_dict()) == {"policy", "value"}


@pytest.fixture(scope="module")
def stop_case():
    """An ungated run whose KL climbs inside the first epoch, and a threshold between two of its KLs."""
    from isaac_rover_orbit_amd.ppo_skrl import TorchSkrlPPO
    ex = load_example()
    B, E, M = 203, 3, 5
    nets = _pair(ex, 2)
    data, perms = _cpu_rollout(*nets, B, seed=4), _perms(B, E, 6)

    def run(**kw):
        t = TorchSkrlPPO(*_clone(ex, nets), lr=1e-2, epochs=E, minibatches=M, device="cpu")
        obs, act, logp, v, ret, adv = data
        vs, rs = t.standardize_values(v, ret)
        return t, t.update(obs, act, logp, vs, rs, adv, perms=perms, **kw)

    free, _ = run()
    k0 = free.last_kls[0]
    j = next(j for j in range(1, M) if k0[j] > max(k0[:j]))                            # the first KL above everything before it
    thr = 0.5 * (k0[j] + max(k0[:j]))
    return dict(run=run, free=free, j=j, thr=thr, perms=perms, B=B, E=E, M=M)


def test_a_stop_skips_the_step_and_the_rest_of_the_epoch(stop_case):
    c = stop_case
    t, (kls, lr) = c["run"](kl_early_stop=c["thr"], scheduler=None)
    rec, stp = t.last_update["recorded"], t.last_update["stopped"]
    assert rec[0] == c["j"] + 1 and stp[0]                                              # the case the threshold was built for
    assert all(r == c["M"] or s for r, s in zip(rec, stp)) and all(1 <= r <= c["M"] for r in rec)
    assert t.steps == sum(r - s for r, s in zip(rec, stp))                              # the stopping minibatch takes no step
    assert t.steps < c["E"] * c["M"]
    # up to the stop the run is the ungated one: the same KLs, the stopping one included, and it is in the epoch's mean
    assert t.last_kls[0] == c["free"].last_kls[0][:c["j"] + 1] and t.last_kls[0][-1] > c["thr"]
    assert all(k <= c["thr"] for k in t.last_kls[0][:-1])
    for e in range(c["E"]):
        assert kls[e] == torch.tensor(t.last_kls[e], dtype=torch.float32).mean().item() and len(t.last_kls[e]) == rec[e]
    # the state scaler trains before the KL is known: on the stopping minibatch too, and on nothing after it
    rows = sum(mb.numel() for mb in c["perms"][0].chunk(c["M"])[:rec[0]])
    assert float(t.state_preprocessor.current_count) == 1 + rows < 1 + c["B"]
    assert float(c["free"].state_preprocessor.current_count) == 1 + c["B"]
    assert lr == 1e-2 == t.lr                                                           # scheduler=None leaves the rate alone


def test_the_comparison_is_strict_and_a_nan_never_stops(stop_case):
    c = stop_case
    k = c["free"].last_kls[0][c["j"]]
    t, _ = c["run"](kl_early_stop=float(np.float32(k)), scheduler=None)
    assert not t.last_update["stopped"][0] or t.last_update["recorded"][0] > c["j"] + 1   # not at the KL equal to the threshold
    assert not (torch.tensor(float("nan")) > 0.008)


def test_scheduler_none_leaves_lr_alone_and_kl_adaptive_moves_it(stop_case):
    c = stop_case
    t, (_, lr) = c["run"](scheduler=None)
    assert lr == 1e-2 and t.last_update == {"recorded": [c["M"]] * c["E"], "stopped": [False] * c["E"]}
    assert c["free"].lr != 1e-2                                                         # the default scheduler moved it
    with pytest.raises(ValueError):
        c["run"](scheduler="linear")


# ------------------------------------------------------------------------------------------------------------- reward shaping
def _shape_inputs(n=37, seed=0):
    g = torch.Generator().manual_seed(seed)
    rew = torch.randn(n, generator=g)
    val = torch.randn(n, generator=g) * 5.0
    trunc = torch.rand(n, generator=g) < 0.4
    rew[0], rew[1] = -0.0, -0.0
    trunc[0], trunc[1] = False, True
    val[2], trunc[2] = float("inf"), False                                              # inf * 0 = nan, as in torch
    val[3], trunc[3] = float("-inf"), True
    return rew, val, trunc


@pytest.mark.parametrize("scale", [1.0, 0.1, -2.5])
@pytest.mark.parametrize("boot", [False, True])
def test_shape_rewards_is_the_torch_expression_bit_for_bit(scale, boot):
    from isaac_rover_orbit_amd.ppo_skrl import shape_rewards
    rew, val, trunc = _shape_inputs()
    keep = rew.clone()
    for tr in (trunc, torch.zeros_like(trunc)):
        got = shape_rewards(rew, val, tr, scale, 0.99, boot)
        want = rew * scale                                                              # skrl: the shaper, then the bootstrap
        if boot:
            want = want + 0.99 * val * tr
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        # the same in numpy float32, every product and the sum rounded once (what the kernel forms)
        r = rew.numpy() * np.float32(scale)
        if boot:
            with np.errstate(invalid="ignore"):
                r = r + (np.float32(0.99) * val.numpy()) * tr.numpy().astype(np.float32)
        assert np.array_equal(got.numpy().view(np.int32), r.view(np.int32))
        if boot:
            assert torch.isnan(got[2]) and (not tr[3] or got[3] == float("-inf"))
        else:
            assert got[2] == rew[2] * scale
        if scale == 1.0:
            assert torch.equal(got[~tr & torch.isfinite(val)], rew[~tr & torch.isfinite(val)])
            # -0.0 stays -0.0 without the bootstrap; with it the sign is that of -0.0 + (0.99 * val) * 0.0, compared above
            assert got[0].item() == 0.0 and (boot or bool(torch.signbit(got[0])))
    assert torch.equal(rew, keep)


def test_torch_rollout_records_shaped_rewards():
    from isaac_rover_orbit_amd import rollout as R
    from isaac_rover_orbit_amd.ppo_skrl import shape_rewards
    n = 9
    ro = R.TorchRollout(lambda o: torch.tanh(o[:, :2]), lambda o: o[:, :1] * 3.0, torch.zeros(2), n, 2, device="cpu")
    g = torch.Generator().manual_seed(1)
    ro.act(0, torch.randn(n, 965, generator=g))
    rew, term, trunc = torch.randn(n, generator=g), torch.arange(n) % 4 == 0, torch.arange(n) % 3 == 0
    ro.record(0, rew, term, trunc, rewards_shaper_scale=0.5, time_limit_bootstrap=True, discount=0.9)
    assert torch.equal(ro.rew[0], shape_rewards(rew, ro.val[0], trunc, 0.5, 0.9, True)) and not torch.equal(ro.rew[0], rew)
    assert torch.equal(ro.done[0], (term | trunc).float())
    ro.record(1, rew, term, trunc)
    assert torch.equal(ro.rew[1], rew)


# ------------------------------------------------------------------------------------------------------------------ the example
def test_example_flags():
    ex = load_example()
    ap = ex.build_parser()
    d = ap.parse_args([])
    assert (d.kl_early_stop, d.scheduler, d.rewards_shaper_scale, d.time_limit_bootstrap) == (0.0, "kl_adaptive", None, False)
    assert (d.update, d.rollout, d.preprocess) == ("torch", "torch", "none")
    a = ap.parse_args(["--kl_early_stop", "0.008", "--scheduler", "none", "--rewards_shaper_scale", "0.1", "--time_limit_bootstrap",
                       "--update", "fused", "--preprocess", "running"])
    assert (a.kl_early_stop, a.scheduler, a.rewards_shaper_scale, a.time_limit_bootstrap) == (0.008, "none", 0.1, True)
    with pytest.raises(SystemExit):
        ap.parse_args(["--scheduler", "linear"])
    text = " ".join(ap.format_help().split())
    assert "--kl_early_stop 0.008 --scheduler none is rover_ppo.yaml as skrl reads it" in text and "rover_rpo.yaml is the same" in text
