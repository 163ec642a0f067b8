"""skrl's KL early stop decided and obeyed on the MI355X (include/rover_train_gate.h, FusedPPO.update(kl_early_stop=, scheduler=)),
the gated scaler train and the shaped record launch.

The oracle for the gate is the UNGATED entry points driven from the host: per minibatch FusedPPO.minibatch, read stats[0] back,
break before FusedPPO.apply where it exceeds the threshold (and, behind the scalers, no state_scaler.train after a stop).  The
all-device gated update must match that run bit for bit.

Where the stop falls is built, not hoped for.  The rollouts have old log-probabilities 0.02 off the networks' own, so a
minibatch's KL is about 2e-4 until the first optimiser step has been taken and a few 1e-2 after it (lr 1e-2: Adam's first step
moves every weight by the rate).  `quiet` minibatches at the head of epoch 0 have zero advantages and run at value_loss_scale 0:
their gradient is exactly zero, Adam's step is 0 / (0 + eps) = 0, and the parameters do not move.  With q quiet minibatches out of
M the first KL past the step is record (0, q + 1), or (1, 0) for q = M - 1.  Each test asserts the case it built, and that every
KL it recorded is a factor 2 away from the threshold."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from rollout_helpers import _biteq
from test_gpu_ppo_update import _nets, _rollout

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, EPOCHS = 1e-2, 3
SHAPES = [(1, 512, 4), (4, 1025, 3), (1, 17, 1)]      # (T, envs, minibatches): 512 rows in 4; 4100 in 1367, 1367, 1366; 17 in one


def _trainer(pol, val, lr=LR, **kw):
    from isaac_rover_orbit_amd.ppo import FusedPPO
    return FusedPPO(pol.state_dict(), val.state_dict(), lr=lr, **kw)


def _f32(x):
    return float(np.float32(x))


def _host_driven(tr, data, perms, mbs, thr, schedule=True, scalers=None, raw=None, image=None):
    """The oracle: ungated entry points, one read-back per minibatch, `break` before apply.  Returns per-epoch KL means, recorded,
    stopped and the (epochs, mbs, 4) stats whose records past a stop still hold NaN."""
    obs, act, logp, v, ret, adv = data
    E = len(perms)
    stats = torch.full((E, mbs, 4), float("nan"), device=DEV)
    kls, recorded, stopped = [], [], []
    for e in range(E):
        rec, stop = 0, False
        for j, mb in enumerate(perms[e].chunk(mbs)):
            mb = mb.contiguous()
            if scalers is not None and e == 0:
                scalers.train(raw, mb)                       # before the KL is known: the stopping minibatch trains too
                scalers.forward(raw, mb, out=image)
            tr.minibatch(image if scalers is not None else obs, act, logp, v, ret, adv, mb, stats=stats[e, j])
            rec += 1
            kl = np.float32(stats[e, j, 0].item())
            if thr > 0 and kl > np.float32(thr):             # strict, fp32
                stop = True
                break
            tr.apply()
        if scalers is not None and e == 0 and E > 1:
            scalers.forward(raw, out=image)
        if schedule:
            out = torch.empty(1, device=DEV)
            tr.kl_schedule(stats[e, :rec].contiguous(), out)  # the parent's mean and rule over the recorded KLs
            kls.append(out.item())
        else:
            s = np.float32(0.0)
            for k in stats[e, :rec, 0].cpu().numpy():
                s = np.float32(s + k)
            kls.append(float(np.float32(s / np.float32(rec))))
        recorded.append(rec); stopped.append(stop)
    return kls, recorded, stopped, stats


def _quiet(data, perms, mbs, q):
    """`data` with zero advantages on the rows of the first q minibatches of epoch 0."""
    obs, act, logp, v, ret, adv = data
    adv = adv.clone()
    for mb in perms[0].chunk(mbs)[:q]:
        adv[mb] = 0.0
    return obs, act, logp, v, ret, adv


def _first_jump(stats, rec):
    """(epoch, record, threshold) of the first recorded KL more than 4x every KL before it, in update order; the threshold is
    the geometric mean of the two sides."""
    seen = []
    for e in range(stats.shape[0]):
        for j in range(rec[e]):
            k = float(stats[e, j, 0])
            if seen and k > 4.0 * max(seen):
                return e, j, math.sqrt(k * max(seen))
            seen.append(k)
    raise AssertionError(f"no KL jumps by a factor 4 in {stats[:, :, 0].tolist()}")


def _gap(stats, rec, thr):
    ks = [float(stats[e, j, 0]) for e in range(stats.shape[0]) for j in range(rec[e])]
    assert all(k < 0.5 * thr or k > 2.0 * thr for k in ks), (thr, ks)


def _assert_same_run(a, b, out_a, out_b):
    """Trainers a (gated, all on the device) and b (host-driven), and what their updates returned."""
    kls_a, rec_a, stp_a, stats_a = out_a
    kls_b, rec_b, stp_b, stats_b = out_b
    assert rec_a == rec_b and stp_a == stp_b, (rec_a, stp_a, rec_b, stp_b)
    assert [_f32(k) for k in kls_a] == [_f32(k) for k in kls_b]
    for name in ("params", "adam_m", "adam_v", "grad", "rep_p", "rep_v"):
        assert _biteq(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.state.view(torch.int64), b.state.view(torch.int64))          # lr, step, norm, clip, step size: every bit
    for e in range(stats_a.shape[0]):
        assert _biteq(stats_a[e, :rec_a[e]], stats_b[e, :rec_a[e]])                   # every recorded record
        assert bool(torch.isnan(stats_a[e, rec_a[e]:]).all())                          # past a stop: the fill, never written
    assert a.steps == sum(r - s for r, s in zip(rec_a, stp_a))


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0] * s[1]}rows-{s[2]}mb")
def shape(request):
    T, n, mbs = request.param
    ex, pol, val = _nets(0)
    data = _rollout(pol, val, T, n, seed=8, lp_noise=0.02, v_noise=0.3)
    B = T * n
    g = torch.Generator(device=DEV).manual_seed(11)
    perms = [torch.randperm(B, device=DEV, generator=g) for _ in range(EPOCHS)]
    free = {}

    def ungated(q):
        """The host-driven run without a threshold on the data with q quiet minibatches: where the KLs come from."""
        if q not in free:
            tr = _trainer(pol, val, **({"value_loss_scale": 0.0} if q else {}))
            free[q] = (tr, _host_driven(tr, _quiet(data, perms, mbs, q), perms, mbs, 0.0))
        return free[q]

    return dict(pol=pol, val=val, data=data, perms=perms, mbs=mbs, B=B, ungated=ungated)


def _both(c, q, thr, scheduler=None):
    """(gated trainer, its outputs, host-driven trainer, its outputs) at threshold thr."""
    kw = {"value_loss_scale": 0.0} if q else {}
    data = _quiet(c["data"], c["perms"], c["mbs"], q)
    host = _trainer(c["pol"], c["val"], **kw)
    out_h = _host_driven(host, data, c["perms"], c["mbs"], thr, schedule=scheduler is not None)
    dev = _trainer(c["pol"], c["val"], **kw)
    kls, lr = dev.update(*data, perms=c["perms"], epochs=EPOCHS, minibatches=c["mbs"], kl_early_stop=thr, scheduler=scheduler)
    assert lr == host.lr == dev.lr
    out_d = (kls, dev.last_update["recorded"], dev.last_update["stopped"], dev.last_stats)
    print(f"thr {thr:.4g} recorded {out_d[1]} stopped {out_d[2]} kls {dev.last_stats[:, :, 0].tolist()}")
    return dev, out_d, host, out_h


@pytest.mark.parametrize("where", ["a_middle", "b_last", "c_first_of_epoch_1"])
def test_gated_update_is_the_host_driven_run_bit_for_bit(shape, where):
    c = shape
    M = c["mbs"]
    q = {"a_middle": 0, "b_last": M - 2, "c_first_of_epoch_1": M - 1}[where]
    if where != "c_first_of_epoch_1" and M < 3:
        q = 0                                   # one minibatch per epoch: the only stop there is falls on (1, 0), first and last at once
    _, (_, rec, _, stats) = c["ungated"](q)
    e, j, thr = _first_jump(stats, rec)
    want = (0, q + 1) if q + 1 < M else (1, 0)
    assert (e, j) == want, (where, e, j, stats[:, :, 0].tolist())                      # the case this test meant to build
    if M >= 3:
        assert {"a_middle": 0 < j < M - 1, "b_last": e == 0 and j == M - 1, "c_first_of_epoch_1": (e, j) == (1, 0)}[where]
    dev, out_d, host, out_h = _both(c, q, thr)
    _assert_same_run(dev, host, out_d, out_h)
    _, rec_d, stp_d, stats_d = out_d
    _gap(stats_d, rec_d, thr)
    assert stp_d[e] and rec_d[e] == j + 1 and not any(stp_d[:e]) and rec_d[:e] == [M] * e
    if (e, j) == (1, 0):
        assert rec_d[1] == 1 and dev.steps == M + sum(r - s for r, s in zip(rec_d[2:], stp_d[2:]))   # one record, no step in epoch 1
    assert dev.lr == LR                                                                  # scheduler=None
    # the epoch state after the update: cleared, counted, and the latest stop described
    ep = dev.epoch_state.cpu()
    last = max(i for i, s in enumerate(stp_d) if s)
    assert ep[:4].tolist() == [0, 0, EPOCHS, sum(stp_d)] and int(ep[4]) == rec_d[last] - 1
    assert _biteq(ep[5:6].view(torch.float32), stats_d[last, rec_d[last] - 1, 0:1].cpu())
    # grad: the stopping minibatch's gradient as rover_ppo_minibatch leaves it, not scaled by a clip coefficient
    if stp_d[-1]:
        fresh = _trainer(c["pol"], c["val"], **({"value_loss_scale": 0.0} if q else {}))
        fresh.params.copy_(dev.params)
        data = _quiet(c["data"], c["perms"], M, q)
        fresh.minibatch(*data, c["perms"][-1].chunk(M)[rec_d[-1] - 1].contiguous())
        assert _biteq(fresh.grad, dev.grad)


def test_a_threshold_above_every_kl_is_the_ungated_update(shape):
    """Case d, under scheduler="kl_adaptive": bit-equal to the host-driven run AND to the ungated update()."""
    c = shape
    _, (_, rec, _, stats) = c["ungated"](0)
    thr = 2.5 * float(stats[:, :, 0].max())
    dev, out_d, host, out_h = _both(c, 0, thr, scheduler="kl_adaptive")
    _assert_same_run(dev, host, out_d, out_h)
    assert out_d[1] == [c["mbs"]] * EPOCHS and out_d[2] == [False] * EPOCHS
    _gap(out_d[3], out_d[1], thr)
    plain = _trainer(c["pol"], c["val"])
    kls_p, lr_p = plain.update(*c["data"], perms=c["perms"], epochs=EPOCHS, minibatches=c["mbs"])
    assert plain.last_update is None
    assert [_f32(k) for k in kls_p] == [_f32(k) for k in out_d[0]] and lr_p == dev.lr
    for name in ("params", "adam_m", "adam_v", "grad", "rep_p", "rep_v"):
        assert _biteq(getattr(plain, name), getattr(dev, name)), name
    assert torch.equal(plain.state.view(torch.int64), dev.state.view(torch.int64))
    assert _biteq(plain.last_stats, dev.last_stats)
    assert dev.epoch_state.cpu().tolist()[:5] == [0, 0, EPOCHS, 0, -1]
    # scheduler=None alone also takes the gated kernels: the same minibatches, the rate's bits kept
    none = _trainer(c["pol"], c["val"])
    none.update(*c["data"], perms=c["perms"], epochs=1, minibatches=c["mbs"], scheduler=None)
    assert none.lr == LR and none.last_update == {"recorded": [c["mbs"]], "stopped": [False]}
    assert _biteq(none.last_stats[0], dev.last_stats[0])


def test_a_kl_equal_to_the_threshold_does_not_stop(shape):
    """Case e: the threshold is a recorded KL's own float32 value; the comparison is strict."""
    c = shape
    _, (_, rec, _, stats) = c["ungated"](0)
    e, j, _ = _first_jump(stats, rec)
    thr = float(stats[e, j, 0])                                                          # exactly representable
    assert _f32(thr) == thr
    dev, out_d, host, out_h = _both(c, 0, thr)
    _assert_same_run(dev, host, out_d, out_h)
    _, rec_d, stp_d, stats_d = out_d
    assert float(stats_d[e, j, 0]) == thr and (rec_d[e] > j + 1 or not stp_d[e])         # recorded, equal, and no stop there
    assert all(not s for s in stp_d[:e])


# ------------------------------------------------------------------------------------------------------- the word itself
def _guarded(n, fill=777.0):
    buf = torch.full((n + 16,), fill, device=DEV)
    return buf, buf[8:8 + n]


def test_a_set_stop_word_leaves_everything_untouched_and_epoch_end_reopens():
    from isaac_rover_orbit_amd.scaler import DeviceScaler
    ex, pol, val = _nets(0)
    obs, act, logp, v, ret, adv = _rollout(pol, val, 1, 100, seed=3, lp_noise=0.02)
    idx = torch.randperm(100, device=DEV)[:37].contiguous()
    tr = _trainer(pol, val, lr=1e-4)                      # below lr_max: the scheduler has room to move it
    tr._ensure_ws(37)
    tr.ws.fill_(0xA5)                                     # stale contents: every float a large negative number
    tr.grad.fill_(777.0)
    sbuf, stats = _guarded(4)
    mbuf, mean_out = _guarded(74)
    vbuf, value_out = _guarded(37)
    sc = DeviceScaler(965, DEV)
    sc.train(obs, idx)                                    # sizes the scaler's workspace
    sc.ws.fill_(0x5A)
    keep = {n: getattr(tr, n).clone() for n in ("params", "grad", "adam_m", "adam_v", "state", "rep_p", "rep_v", "ws")}
    keep_sc = (sc.block.clone(), sc.ws.clone())
    tr.epoch_state[0] = 1
    tr.minibatch_gated(obs, act, logp, v, ret, adv, idx, stats, 0.008, mean_out=mean_out.view(37, 2), value_out=value_out.view(37, 1))
    tr.apply_gated()
    sc.train(obs, idx, gate=tr.epoch_state)
    for n, t in keep.items():
        assert torch.equal(getattr(tr, n).view(torch.uint8), t.view(torch.uint8)), n
    assert all(bool((b == 777.0).all()) for b in (sbuf, mbuf, vbuf)) and tr.steps == 0
    assert torch.equal(sc.block, keep_sc[0]) and torch.equal(sc.ws, keep_sc[1])
    assert tr.epoch_state.cpu().tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    # epoch_end: nothing recorded -> kl 0 and, even with the scheduler on, the rate's bits kept; the word is cleared
    kl = torch.full((1,), 5.0, device=DEV)
    all_stats = torch.full((3, 4), float("nan"), device=DEV)
    tr.epoch_end(all_stats, True, kl)
    assert kl.item() == 0.0 and torch.equal(tr.state.view(torch.int64), keep["state"].view(torch.int64))
    assert tr.epoch_state.cpu().tolist()[:5] == [0, 0, 1, 1, 0]
    # ... and the next minibatch runs again, over the stale workspace, as the ungated entries do on a fresh trainer
    fresh = _trainer(pol, val, lr=1e-4)
    fs = fresh.minibatch(obs, act, logp, v, ret, adv, idx)
    fresh.apply()
    tr.minibatch_gated(obs, act, logp, v, ret, adv, idx, stats, 0.0, mean_out=mean_out.view(37, 2), value_out=value_out.view(37, 1))
    tr.apply_gated()
    assert _biteq(stats, fs) and bool((sbuf[:8] == 777.0).all()) and bool((sbuf[12:] == 777.0).all())
    assert bool((mbuf[:8] == 777.0).all()) and bool((mbuf[82:] == 777.0).all()) and bool((mean_out != 777.0).all())
    for n in ("params", "grad", "adam_m", "adam_v", "rep_p", "rep_v"):
        assert _biteq(getattr(tr, n), getattr(fresh, n)), n
    assert torch.equal(tr.state.view(torch.int64), fresh.state.view(torch.int64)) and tr.steps == 1
    assert tr.epoch_state.cpu().tolist()[:4] == [0, 1, 1, 1]                             # threshold 0: recorded, never a stop
    # schedule = 0 keeps lr's bits; schedule = 1 is rover_ppo_kl_schedule's rule on the recorded mean
    all_stats[0] = stats
    lr_bits = tr.state.view(torch.int64)[0].item()
    tr.epoch_end(all_stats, False, kl)
    assert tr.state.view(torch.int64)[0].item() == lr_bits and _biteq(kl, stats[0:1])
    fresh.kl_schedule(all_stats[:1].contiguous(), None)
    tr.epoch_state[1] = 1
    tr.epoch_end(all_stats, True, kl)
    assert tr.state.view(torch.int64)[0].item() == fresh.state.view(torch.int64)[0].item() != lr_bits
    # an open gate: the gated scaler train is the ungated one
    sc2 = DeviceScaler(965, DEV)
    sc2.train(obs, idx)
    sc2.train(obs, idx)
    sc.train(obs, idx, gate=tr.epoch_state)
    assert torch.equal(sc.block.view(torch.int64), sc2.block.view(torch.int64))


# ------------------------------------------------------------------------------------------------------- behind the scalers
def _scaled_inputs(pol, val, T, n_env, seed=8):
    """tests/test_gpu_ppo_scaled.py's `_inputs` with old log-probabilities 0.02 off the networks' own."""
    from test_gpu_ppo_scaled import _Doubled
    obs, act, logp, oldv, ret, adv = _rollout(_Doubled(pol), _Doubled(val), T, n_env, seed=seed, lp_noise=0.02, v_noise=0.3)
    g = torch.Generator(device=DEV).manual_seed(seed + 100)
    col = torch.rand(965, device=DEV, generator=g)
    raw = (obs * (0.2 + 4.0 * col) + (col - 0.5) * 6.0).contiguous()
    return raw, act, logp, (oldv * 3.0 + 5.0).contiguous(), (ret * 3.0 + 5.0).contiguous(), adv


@pytest.fixture(scope="module")
def scaled_case():
    """4096 rows in 4 minibatches (tests/test_gpu_ppo_scaled.py's first case), case (a) in epoch 0 from an ungated host run."""
    from isaac_rover_orbit_amd.ppo_scaled import FusedScaledPPO
    ex, pol, val = _nets(0)
    raw, act, logp, oldv, ret, adv = _scaled_inputs(pol, val, 8, 512)
    B, M = 4096, 4
    g = torch.Generator(device=DEV).manual_seed(12)
    perms = [torch.randperm(B, device=DEV, generator=g) for _ in range(EPOCHS)]

    def host(thr):
        tr = FusedScaledPPO(pol.state_dict(), val.state_dict(), lr=LR)
        val_s, ret_s = tr.standardize_values(oldv, ret)
        image = torch.empty(B, 965, device=DEV)
        out = _host_driven(tr.inner, (None, act, logp, val_s, ret_s, adv), perms, M, thr, schedule=False, scalers=tr.state_scaler,
                           raw=raw, image=image)
        return tr, out, image

    _, (_, rec, _, stats), _ = host(0.0)
    e, j, thr = _first_jump(stats, rec)
    assert e == 0 and 0 < j < M - 1, (e, j, stats[:, :, 0].tolist())                   # case (a), in the epoch that trains the scaler
    p0 = {r: {k: v.detach().cpu().clone() for k, v in net.state_dict().items()} for r, net in (("policy", pol), ("value", val))}
    return dict(ex=ex, pol=pol, val=val, data=(raw, act, logp, oldv, ret, adv), perms=perms, B=B, M=M, thr=thr, j=j, host=host, p0=p0)


def test_scaled_gated_update_is_the_host_driven_run(scaled_case):
    from isaac_rover_orbit_amd.ppo_scaled import FusedScaledPPO
    c = scaled_case
    raw, act, logp, oldv, ret, adv = c["data"]
    host, out_h, image_h = c["host"](c["thr"])
    tr = FusedScaledPPO(c["pol"].state_dict(), c["val"].state_dict(), lr=LR)
    keep = raw.clone()
    val_s, ret_s = tr.standardize_values(oldv, ret)
    kls, lr = tr.update(raw, act, logp, val_s, ret_s, adv, perms=c["perms"], epochs=EPOCHS, minibatches=c["M"],
                        kl_early_stop=c["thr"], scheduler=None)
    assert torch.equal(raw, keep) and lr == LR
    out_d = (kls, tr.last_update["recorded"], tr.last_update["stopped"], tr.inner.last_stats)
    print(f"thr {c['thr']:.4g} recorded {out_d[1]} stopped {out_d[2]} kls {out_d[3][:, :, 0].tolist()}")
    _assert_same_run(tr.inner, host.inner, out_d, out_h)
    _gap(out_d[3], out_d[1], c["thr"])
    assert out_d[1][0] == c["j"] + 1 and out_d[2][0]
    # the state scaler trained on the recorded minibatches of epoch 0, the stopping one included, and on nothing else
    rows = sum(mb.numel() for mb in c["perms"][0].chunk(c["M"])[:c["j"] + 1])
    assert float(tr.state_scaler.current_count) == 1 + rows < 1 + c["B"]
    assert torch.equal(tr.state_scaler.block.view(torch.int64), host.state_scaler.block.view(torch.int64))
    assert torch.equal(tr.value_scaler.block.view(torch.int64), host.value_scaler.block.view(torch.int64))
    # after the update the image holds the final statistics' rows
    assert _biteq(tr._image[:c["B"]], tr.state_scaler.forward(raw)) and _biteq(tr._image[:c["B"]], image_h)


def _spec_run(c, dtype, device):
    from isaac_rover_orbit_amd.ppo_skrl import TorchSkrlPPO
    ex = c["ex"]
    p, v = ex.Net(2, True), ex.Net(1, False)
    p.load_state_dict(c["pol"].state_dict()); v.load_state_dict(c["val"].state_dict())
    tp = TorchSkrlPPO(p.to(dtype), v.to(dtype), lr=LR, epochs=EPOCHS, minibatches=c["M"], device=device)
    raw, act, logp, oldv, ret, adv = (x.to(device=device, dtype=dtype) for x in c["data"])
    val_s, ret_s = tp.standardize_values(oldv, ret)
    kls, lr = tp.update(raw, act, logp, val_s, ret_s, adv, perms=[q.to(device) for q in c["perms"]], kl_early_stop=c["thr"], scheduler=None)
    return tp, kls, lr


def test_scaled_gated_update_tracks_the_skrl_spec(scaled_case):
    """tests/test_gpu_ppo_scaled.py's protocol at case (a).  The bound is the specification's own float32-against-float64 distance
    on these inputs, times 4 (the allowance tests/test_gpu_ppo_update.py gives the fused gradients over torch's float32 error):
    the step error in norm, and the epoch KLs with a floor of 1e-4 relative -- a KL term (r - 1) - log r is about x^2 / 2 with
    x = log r, the difference of two numbers of size |x| each carrying float32's 6e-8, so its relative error is about 2.4e-7 / |x|,
    1e-5 at the |x| = 0.02 these rollouts start from; the floor leaves a factor 10.  Measured on an MI355X: step error against
    the float64 spec 7.1e-5 fused, 9.1e-5 the spec in float32 (step norm 5.63); epoch KLs 5.5e-7 relative fused, 4.3e-7 the spec."""
    from isaac_rover_orbit_amd.ppo_scaled import FusedScaledPPO
    from test_gpu_ppo_scaled import _step_error
    c = scaled_case
    t64, k64, _ = _spec_run(c, torch.float64, "cpu")
    t32, k32, _ = _spec_run(c, torch.float32, DEV)
    # the float64 specification makes the decisions the threshold was built for, with the factor-2 gap
    assert t64.last_update["recorded"][0] == c["j"] + 1 and t64.last_update["stopped"][0]
    ks = [k for e in t64.last_kls for k in e]
    assert all(k < 0.5 * c["thr"] or k > 2.0 * c["thr"] for k in ks), (c["thr"], ks)
    tr = FusedScaledPPO(c["pol"].state_dict(), c["val"].state_dict(), lr=LR)
    raw, act, logp, oldv, ret, adv = c["data"]
    val_s, ret_s = tr.standardize_values(oldv, ret)
    kf, lrf = tr.update(raw, act, logp, val_s, ret_s, adv, perms=c["perms"], epochs=EPOCHS, minibatches=c["M"], kl_early_stop=c["thr"],
                        scheduler=None)
    assert tr.last_update == t64.last_update == t32.last_update and tr.steps == t64.steps == t32.steps
    assert lrf == t64.lr == LR
    n32, den = _step_error(t32.state_dict(), t64.state_dict(), c["p0"])
    nf, _ = _step_error(tr.state_dict(), t64.state_dict(), c["p0"])
    rel32 = max(abs(a - b) / abs(b) for a, b in zip(k32, k64))
    relf = max(abs(a - b) / abs(b) for a, b in zip(kf, k64))
    print(f"step error: spec32 {n32:.3e}, fused {nf:.3e} of {den:.3e}; KL rel: spec32 {rel32:.3e}, fused {relf:.3e}; kls {kf} / {k64}")
    assert nf <= 4.0 * n32, (nf, n32, den)
    assert relf <= max(4.0 * rel32, 1e-4), (relf, rel32)


# ------------------------------------------------------------------------------------------------------------- the record
@pytest.mark.parametrize("n", [1, 255, 257])
def test_record_shaped_is_shape_rewards_bit_for_bit(n):
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd.ppo_skrl import shape_rewards
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(n)
    f = lambda: torch.zeros(n + 9, device=DEV)  # noqa: E731
    rew_b, val_b = f(), f()
    rew, val = rew_b[1:1 + n], val_b[1:1 + n]                                            # 4 bytes off 16-byte alignment
    rew.copy_(torch.randn(n, device=DEV, generator=g)); val.copy_(torch.randn(n, device=DEV, generator=g) * 5.0)
    flags = torch.zeros(2, n + 9, dtype=torch.uint8, device=DEV)
    term, trunc = flags[0, 1:1 + n], flags[1, 3:3 + n]
    term.copy_(torch.rand(n, device=DEV, generator=g) < 0.3); trunc.copy_(torch.rand(n, device=DEV, generator=g) < 0.4)
    rew[0] = -0.0
    if n > 4:
        val[2], trunc[2] = float("inf"), 0                                               # inf * 0 = nan, as in torch
        val[3], trunc[3] = float("-inf"), 1
        rew[4], trunc[4], term[4] = -0.0, 1, 0
    assert rew.data_ptr() % 16 == 4 and val.data_ptr() % 16 == 4
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    plain_r, plain_d = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    _lib.check(lib.rover_rollout_record(rew.data_ptr(), term.data_ptr(), trunc.data_ptr(), n, plain_r.data_ptr(), plain_d.data_ptr(),
                                        stream), "rover_rollout_record")
    for scale, disc, boot in ((1.0, 0.99, True), (0.1, 0.99, True), (-2.5, 0.9, True), (0.1, 0.99, False), (1.0, 0.99, False)):
        ob = torch.full((2, n + 9), 777.0, device=DEV)
        ro, do = ob[0, 1:1 + n], ob[1, 1:1 + n]
        assert ro.data_ptr() % 16 == 4
        _lib.check(lib.rover_rollout_record_shaped(rew.data_ptr(), term.data_ptr(), trunc.data_ptr(), val.data_ptr() if boot else None, n,
                                                   scale, disc, int(boot), ro.data_ptr(), do.data_ptr(), stream),
                   "rover_rollout_record_shaped")
        want = shape_rewards(rew.cpu(), val.cpu(), trunc.cpu().bool(), scale, disc, boot)
        assert _biteq(ro.cpu(), want), (scale, disc, boot)
        assert _biteq(do, plain_d)
        assert bool((ob[:, 0] == 777.0).all()) and bool((ob[:, 1 + n:] == 777.0).all())  # the guards
        if boot and n > 4:
            assert bool(torch.isnan(ro[2])) and ro[3].item() == float("-inf")
        if not boot and scale == 1.0:
            assert _biteq(ro, plain_r)


def test_collectors_record_through_the_shaped_launch():
    from isaac_rover_orbit_amd.ppo_skrl import shape_rewards
    from isaac_rover_orbit_amd.rollout import RolloutCollector
    from rollout_helpers import make_nets, synthetic_rows
    n = 33
    nets = make_nets(2)
    col = RolloutCollector(nets[0], nets[1], torch.tensor([-0.4, 0.3], device=DEV), n, 2)
    col.act(0, synthetic_rows(n, seed=1))
    g = torch.Generator(device=DEV).manual_seed(5)
    rew = torch.randn(n, device=DEV, generator=g)
    term, trunc = torch.rand(n, device=DEV, generator=g) < 0.3, torch.rand(n, device=DEV, generator=g) < 0.5
    col.record(0, rew, term, trunc, rewards_shaper_scale=0.1, time_limit_bootstrap=True, discount=0.99)
    assert _biteq(col.rew[0].cpu(), shape_rewards(rew.cpu(), col.val[0].cpu(), trunc.cpu(), 0.1, 0.99, True))
    assert bool(trunc.any()) and not torch.equal(col.rew[0], rew * 0.1)
    assert torch.equal(col.done[0], (term | trunc).float())
    col.record(1, rew, term, trunc)                                                      # the defaults: the plain launch
    assert _biteq(col.rew[1], rew)
    col.record(1, rew, term, trunc, rewards_shaper_scale=0.5)                            # scale alone: val is not read
    assert _biteq(col.rew[1].cpu(), rew.cpu() * 0.5)
