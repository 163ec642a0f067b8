"""The lift task's fused rollout step (include/rover_lift_rollout.h) on the MI355X at the branches tests/test_gpu_lift_rollout.py
does not reach: action widths other than 8, rows past n, every pointer alignment, the number of weight replicas, non-finite rows,
hyper-parameters and scaler blocks away from their defaults, ids / seeds / counters at the top of their ranges, a side stream, the
record kernel on raw bytes and non-finite values, and collector slots at a ragged shape.  No case has more than 257 rows; every
launch writes between sentinel guard rows.  The case lists live in tests/lift_rollout_helpers.py and run on the specification in
tests/test_lift_rollout.py.  Bounds:

  * obs_out, mean, val, env_act: BIT-EXACT (the raw rows; ``actor(trainer.standardize(o))`` and ``trainer.standardize(critic(s),
    "value", inverse=True)``, the generic forward kernel; ``act.clamp``), NaN positions compared as a mask where a case has them
  * mean / val in the width and scaler cases also against a float64 forward of a float64 standardisation: 1e-5 * max(1, |ref|.max())
    (tests/test_gpu_lift_ppo.py::test_elu_forward_matches_float64); rows with a standardised value within 1e-6 of +-clip before the
    clamp are left out (at most 5 % of a case's rows, checked on the CPU in tests/test_lift_rollout.py as well)
  * eps: 2.05e-06 against the float64 Box-Muller spec; act: 4 ulp of max(|mean|, |std * eps|); logp: (8 + (A - 2) / 2) * 2**-23 of
    sum_c (0.5 x_c**2 + |ls_c| + 0.919), A = 1 as A = 2; each maximum is printed before it is asserted
"""
import ctypes as C

import numpy as np
import pytest
import torch

import lift_rollout_helpers as H
from lift_rollout_helpers import FILL, GUARD, OUT_KEYS, TAG, _biteq, _make_trainer, _run, same_bits_nan_aware

pytestmark = pytest.mark.gpu

HP_FIELDS = ("log_std_min", "log_std_max", "scaler_eps", "scaler_clip")


@pytest.fixture(scope="module")
def trainer():
    return _make_trainer()


@pytest.fixture(scope="module")
def nets_of(trainer):
    cache = {}

    def get(A):
        if A not in cache:
            cache[A] = H.WidthNets(A, trainer)
        return cache[A]
    return get


def _rows(n, seed=0):
    return H.lift_rows(n, seed).cuda()


def _reference(tr, o):
    """(mean, val) of the generic forward kernel on the trainer's standardised rows: the contract of the header."""
    s = tr.standardize(o)
    return tr.actor(s), tr.standardize(tr.critic(s), "value", inverse=True)


def _filled(n, A):
    return {k: torch.full(s, FILL, device="cuda") for k, s in H._shapes(n, A).items()}


def _launch(tr, o, outs, counter=0, **hp):
    from isaac_rover_orbit_amd import lift_rollout as LR
    LR.lift_rollout_act(tr.actor, tr.critic, tr.log_std, o, counter, H.hparams_of(**hp), tr.state_scaler, tr.value_scaler,
                        **{k + "_out": outs.get(k) for k in OUT_KEYS})
    torch.cuda.synchronize()
    return outs


def _refused(tr, o, match="code 1", outs=None, **hp):
    """The host-side checks return before a launch: a RoverHipError with the code, every output still at its fill."""
    from isaac_rover_orbit_amd import _lib
    outs = _filled(o.shape[0], tr.actor.out_dim) if outs is None else outs
    before = {k: v.clone() for k, v in outs.items()}
    with pytest.raises(_lib.RoverHipError, match=match):
        _launch(tr, o, outs, **hp)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert _biteq(v, before[k]), k


def _abi_act(tr, obs_ptr, n, outs, h=None, state_ptr=None, value_ptr=None):
    """rover_lift_rollout_act itself, for arguments the wrapper cannot form (n = 0, a scaler block 4 bytes off): the return code."""
    from isaac_rover_orbit_amd import _lib
    p = lambda k: outs[k].data_ptr()      # noqa: E731
    h = H.hparams_of() if h is None else h
    return _lib.load().rover_lift_rollout_act(
        C.byref(tr.actor.desc), tr.actor.packed.data_ptr(), C.byref(tr.critic.desc), tr.critic.packed.data_ptr(), tr.actor.n_copies,
        C.byref(h), C.c_uint64(0), obs_ptr, n, tr.log_std.data_ptr(), state_ptr or tr.state_scaler.data_ptr(),
        value_ptr or tr.value_scaler.data_ptr(), p("obs"), p("mean"), p("val"), p("act"), p("env_act"), p("logp"), p("eps"),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _untouched(outs):
    torch.cuda.synchronize()
    return all(bool((v == FILL).all()) for v in outs.values())


def _ls_clamped(log_std, lo=-20.0, hi=2.0):
    return np.clip(log_std.detach().cpu().numpy().astype(np.float64), lo, hi)


# ------------------------------------------------------------------------------------------------------------ 1. action widths
@pytest.mark.parametrize("n", H.WIDTH_ROWS)
@pytest.mark.parametrize("A", H.WIDTHS)
def test_action_widths(trainer, nets_of, A, n):
    from isaac_rover_orbit_amd import rollout as R
    nets = nets_of(A)
    o = _rows(n, seed=n)
    out = _run(nets, o, counter=5, seed_lo=9, env_id_offset=11, clip_actions=1)
    mean, val = _reference(nets, o)
    assert mean.shape == (n, A) and val.shape == (n, 1)
    assert _biteq(out["obs"], o) and _biteq(out["mean"], mean) and _biteq(out["val"], val)
    assert torch.isfinite(mean).all() and torch.isfinite(val).all() and _biteq(out["env_act"], out["act"].clamp(-1.0, 1.0))
    H.check_float64(out, H.float64_forward(nets.sd_p, nets.sd_v, o, nets.state_scaler, nets.value_scaler, 1e-8, 5.0), f"A={A} n={n}")
    ls_raw = H.log_std_of(A)
    assert (ls_raw > 2.0).any() and (A == 1 or (ls_raw < -20.0).any())
    H.check_sampling(out, n, np.clip(ls_raw.astype(np.float64), -20.0, 2.0), f"A={A} n={n}", counter=5, seed=9, offset=11)
    if A % 2:     # the odd last column is the cosine draw of pair (A - 1) / 2
        pair = R.standard_normals(9, 11 + np.arange(n), 5, 2, tag=TAG | ((A - 1) // 2))[:, 0]
        d = float(np.abs(out["eps"][:, A - 1].double().cpu().numpy() - pair).max())
        print(f"A={A} n={n}: last column against the cosine draw of pair {(A - 1) // 2}: {d:.3e}")
        assert d <= H.EPS_TOL
    if A < H.MAX_WIDTH:     # nesting: the actor of width A + 1 is this one plus an appended output row
        wider = nets_of(A + 1)
        ls = torch.cat([nets.log_std, nets.log_std.new_tensor([0.1])])
        o1 = _run(wider, o, counter=5, seed_lo=9, env_id_offset=11, clip_actions=1, log_std=ls)
        for k in ("mean", "eps", "act"):
            assert _biteq(o1[k][:, :A], out[k]), k


def test_width_17_is_refused(trainer):
    from isaac_rover_orbit_amd import lift_rollout as LR
    nets = H.WidthNets(H.MAX_WIDTH + 1, trainer)
    assert nets.actor.out_dim == 17
    _refused(nets, _rows(17), match="code 4")                       # ROVER_ERR_UNSUPPORTED: more than one column tile
    with pytest.raises(ValueError):
        LR.LiftRolloutCollector(nets, 17, 1)


# -------------------------------------------------------------------------------------------------------------- 2. rows past n
@pytest.mark.parametrize("n", [1, 15, 17, 33])
@pytest.mark.parametrize("A", [2, 16])
def test_nothing_is_written_or_read_past_n(nets_of, A, n):
    nets = nets_of(A)
    o = _rows(n, seed=40 + n)
    plain = _run(nets, o.clone(), counter=8, env_id_offset=3, clip_actions=1)
    src = torch.full((GUARD + n, H.OBS), H.NAN, device="cuda")       # obs: the LAST n rows of its allocation, NaN rows in front
    src[GUARD:] = o
    out = _run(nets, src[GUARD:], counter=8, env_id_offset=3, clip_actions=1)       # _run holds the guards around every output
    for k in OUT_KEYS:
        assert _biteq(out[k], plain[k]), k
        assert torch.isfinite(out[k]).all(), k
    assert torch.isnan(src[:GUARD]).all()


# -------------------------------------------------------------------------------------------------------- 3. alignment matrix
def _offset_views(n, A, offsets):
    """Every output as a view that starts ``offsets[key]`` floats into a larger flat buffer filled with FILL."""
    bufs, views = {}, {}
    for k, shape in H._shapes(n, A).items():
        numel, off = int(np.prod(shape)), offsets[k]
        bufs[k] = torch.full((numel + 8,), FILL, device="cuda")
        views[k] = bufs[k][off:off + numel].view(shape)
        assert views[k].is_contiguous() and views[k].data_ptr() % 16 == (bufs[k].data_ptr() + 4 * off) % 16
    return bufs, views


@pytest.mark.parametrize("n", [16, 17, 32])
@pytest.mark.parametrize("A", [3, 8])
def test_alignment_matrix(trainer, nets_of, A, n):
    nets = trainer if A == 8 else nets_of(A)
    o = _rows(n, seed=50 + n)
    ref = _run(nets, o, counter=4, clip_actions=1)
    mixed = {"in": 1, "obs": 3, "mean": 2, "val": 1, "act": 3, "env_act": 0, "logp": 1, "eps": 2}
    for offsets in [dict.fromkeys(mixed, d) for d in (1, 2, 3)] + [mixed]:
        src = torch.full((n * H.OBS + 8,), H.NAN, device="cuda")
        obs = src[offsets["in"]:offsets["in"] + n * H.OBS].view(n, H.OBS)
        obs.copy_(o)
        assert obs.data_ptr() % 16 == (src.data_ptr() + 4 * offsets["in"]) % 16 and src.data_ptr() % 16 == 0
        bufs, views = _offset_views(n, A, offsets)
        _launch(nets, obs, views, counter=4, clip_actions=1)
        for k in OUT_KEYS:
            assert _biteq(views[k], ref[k]), (offsets[k], k)
            off, numel = offsets[k], views[k].numel()
            assert (bufs[k][:off] == FILL).all() and (bufs[k][off + numel:] == FILL).all(), (offsets[k], k)


def test_misaligned_scaler_blocks_and_weights_are_refused(trainer):
    from isaac_rover_orbit_amd.policy import RoverNet
    n = 17
    o = _rows(n)
    outs = _filled(n, 8)
    for blk, key in ((trainer.state_scaler, "state_ptr"), (trainer.value_scaler, "value_ptr")):
        words = blk.view(torch.float32)
        shifted = torch.zeros(words.numel() + 3, device="cuda")     # the same bytes, 4 bytes off an 8-byte boundary
        shifted[1:1 + words.numel()] = words
        ptr = shifted.data_ptr() + 4
        assert ptr % 8 == 4
        assert _abi_act(trainer, o.data_ptr(), n, outs, **{key: ptr}) == 1 and _untouched(outs)       # ROVER_ERR_INVALID
    assert _abi_act(trainer, o.data_ptr(), n, outs) == 0                                               # the same call, aligned
    torch.cuda.synchronize()
    assert _biteq(outs["mean"], _reference(trainer, o)[0])

    class Shifted:
        log_std, state_scaler, value_scaler, critic = trainer.log_std, trainer.state_scaler, trainer.value_scaler, trainer.critic
    packed = trainer.actor.packed
    buf = torch.zeros(packed.numel() + 4, device="cuda")
    buf[1:1 + packed.numel()] = packed
    Shifted.actor = RoverNet.from_packed(trainer.actor.desc, buf[1:1 + packed.numel()], trainer.actor.n_copies)
    assert Shifted.actor.packed.data_ptr() % 16 == 4
    _refused(Shifted, o, match="code 1")


# ----------------------------------------------------------------------------------------------------------- 4. weight replicas
@pytest.fixture(scope="module")
def replica_reference():
    tr = _make_trainer(n_copies=1)
    return {n: _run(tr, _rows(n, seed=60 + n), counter=2, clip_actions=1) for n in (17, 257)}


@pytest.mark.parametrize("n_copies", [1, 2, 3, 5, 32])
def test_number_of_weight_replicas(replica_reference, n_copies):
    tr = _make_trainer(n_copies=n_copies)
    assert tr.actor.n_copies == tr.critic.n_copies == n_copies and tr.rep_p.numel() == n_copies * tr.n_p
    other = _make_trainer(seed=4)                                   # different weights for one replica
    for n in (17, 257):
        o = _rows(n, seed=60 + n)
        blocks = (n + 15) // 16
        base = _run(tr, o, counter=2, clip_actions=1)
        for k in OUT_KEYS:
            assert _biteq(base[k], replica_reference[n][k]), (n, k)
        for k in sorted(k for k in {1, n_copies - 1} if 0 < k < n_copies):
            keep_p, keep_v = tr.rep_p.clone(), tr.rep_v.clone()
            tr.rep_p[k * tr.n_p:(k + 1) * tr.n_p] = other.params[:tr.n_p]
            tr.rep_v[k * tr.n_v:(k + 1) * tr.n_v] = other.params[tr.n_p:tr.n_p + tr.n_v]
            moved = _run(tr, o, counter=2, clip_actions=1)
            tr.rep_p.copy_(keep_p); tr.rep_v.copy_(keep_v)
            hit = [b for b in range(blocks) if b % n_copies == k]
            assert hit or k >= blocks
            for b in range(blocks):
                rows = slice(16 * b, min(16 * b + 16, n))
                for key in ("mean", "val", "act", "env_act", "logp"):
                    same = _biteq(moved[key][rows], base[key][rows])
                    if b not in hit:
                        assert same, (n, k, b, key)
                    elif key in ("mean", "val", "act"):     # logp depends on act - mean only, env_act may sit at a bound
                        assert not same, (n, k, b, key)
                if b in hit:     # every row of the block reads the overwritten replica
                    assert (moved["mean"][rows] != base["mean"][rows]).any(1).all() and (moved["val"][rows] != base["val"][rows]).all()
            assert _biteq(moved["eps"], base["eps"]) and _biteq(moved["obs"], base["obs"])


# ----------------------------------------------------------------------------------------------------------- 5. non-finite rows
@pytest.mark.parametrize("clip_actions", [0, 1])
@pytest.mark.parametrize("n", H.POISON_ROWS)
def test_non_finite_rows(trainer, n, clip_actions):
    """A NaN in row r poisons row r's mean, val, act, env_act and logp only; +-inf standardises to +-clip.  With clip_actions = 1 the
    NaN has to pass the clamp as it passes torch.clamp: fminf(fmaxf(a, low), high) alone returned action_low here."""
    from isaac_rover_orbit_amd import rollout as R
    o = _rows(n, seed=70 + n)
    raw, nan_rows, inf_rows = H.poison(o)
    kw = dict(counter=6, seed_lo=7, env_id_offset=3, clip_actions=clip_actions)
    out, clean = _run(trainer, raw, **kw), _run(trainer, o, **kw)
    ea = out["env_act"][nan_rows]
    print(f"n={n} clip_actions={clip_actions}: env_act of the NaN rows {nan_rows}: {int(torch.isnan(ea).sum())} of {ea.numel()} NaN, "
          f"{int((ea == -1.0).sum())} at action_low")
    eps64 = R.standard_normals(7, 3 + np.arange(n), 6, 8, tag=TAG)
    H.check_poisoned(out, clean, raw, nan_rows, inf_rows, eps64)
    mean, val = _reference(trainer, raw)
    assert same_bits_nan_aware(out["mean"], mean) and same_bits_nan_aware(out["val"], val)
    assert torch.isfinite(mean[inf_rows]).all() and torch.isfinite(val[inf_rows]).all()
    assert (trainer.standardize(raw)[inf_rows].abs().max(1).values == 5.0).all()
    want = out["act"].clamp(-1.0, 1.0) if clip_actions else out["act"]
    assert same_bits_nan_aware(out["env_act"], want)


# ------------------------------------------------------------------------------------------------------- 6. hyper-parameters
HP_CASES = {"eps_0": dict(scaler_eps=0.0), "eps_1e-2": dict(scaler_eps=1e-2), "clip_0": dict(scaler_clip=0.0),
            "clip_0.5": dict(scaler_clip=0.5), "clip_1e30": dict(scaler_clip=1e30),
            "window": dict(log_std_min=H.WINDOWS[0][0], log_std_max=H.WINDOWS[0][1]),
            "window_min_eq_max": dict(log_std_min=H.WINDOWS[1][0], log_std_max=H.WINDOWS[1][1])}


@pytest.mark.parametrize("name", sorted(HP_CASES))
def test_hyper_parameters_away_from_the_defaults(name):
    from isaac_rover_orbit_amd import lift_rollout as LR
    kw = HP_CASES[name]
    tr = _make_trainer(**kw)
    n = 33
    col = LR.LiftRolloutCollector(tr, n, 1, seed=5)
    h = col.hparams()
    hp = {f: getattr(h, f) for f in HP_FIELDS}                       # what the collector passes on
    for f, v in kw.items():
        assert hp[f] == np.float32(v), f
    eps, clip = hp["scaler_eps"], hp["scaler_clip"]
    # -- mean / val on rows that reach the scaler's edges: the variance-0 column at its mean (0 / eps; NaN at eps 0) and away from it
    o = _rows(n, seed=80)
    if name != "clip_0":     # at clip 0 every value is "near the clamp boundary" of the float64 comparison when it is 0
        o[::3, 7] = float(tr.state_scaler[7])
    out = _run(tr, o, counter=1, seed_lo=5, **hp)
    mean, val = _reference(tr, o)
    assert same_bits_nan_aware(out["mean"], mean) and same_bits_nan_aware(out["val"], val) and _biteq(out["obs"], o)
    s = tr.standardize(o)
    if name == "eps_0":
        assert torch.isnan(s[::3, 7]).all() and (s[1::3, 7].abs() == 5.0).all() and torch.isnan(out["mean"][::3]).all()
        assert torch.isfinite(out["mean"][1::3]).all()
    else:
        assert torch.isfinite(out["mean"]).all() and torch.isfinite(out["val"]).all()
    if name == "clip_0":
        assert (s == 0).all() and _biteq(out["mean"], out["mean"][:1].expand(n, 8))
    if name == "clip_1e30":
        assert float(s.abs().max()) > 1e6
    if "scaler" in next(iter(kw)):
        sd = tr.state_dict()
        H.check_float64(out, H.float64_forward(sd["policy"], sd["value"], o, tr.state_scaler, tr.value_scaler, eps, clip), name)
    # -- act / logp on finite rows, ls clamped to the trainer's window; the update re-evaluates the rows to a KL entry of exactly 0
    o = _rows(n, seed=81)
    col.act(0, o)
    out = _run(tr, o, counter=0, seed_lo=5, **hp)
    for k, buf in (("obs", col.obs), ("mean", col.mean), ("act", col.actions), ("logp", col.logp)):
        assert _biteq(buf[0], out[k]), k
    H.check_sampling(out, n, _ls_clamped(tr.log_std, hp["log_std_min"], hp["log_std_max"]), name, seed=5)
    idx = torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    g = torch.Generator(device="cuda").manual_seed(4)
    adv, ret = torch.randn(n, device="cuda", generator=g), torch.randn(n, device="cuda", generator=g)
    stats = tr.minibatch(col.obs[0], col.actions[0], col.logp[0], col.val[0], ret, adv, idx, train_scaler=False)
    torch.cuda.synchronize()
    print(f"{name}: KL entry {float(stats[0])!r}")
    assert float(stats[0]) == 0.0


def test_refusals_leave_the_outputs_untouched(trainer):
    n = 17
    o = _rows(n)
    base = _run(trainer, o, counter=3)
    _refused(trainer, o, log_std_min=3.0)                           # log_std_min > log_std_max
    _refused(trainer, o, clip_actions=1, action_low=1.0, action_high=-1.0)
    _refused(trainer, o, scaler_clip=-1.0)
    _refused(trainer, o, scaler_clip=H.NAN)
    _refused(trainer, o, log_std_min=H.NAN)
    outs = _filled(n, 8)
    outs["obs"] = o                                                  # obs_out aliasing obs
    _refused(trainer, o, outs=outs)
    outs = _filled(n, 8)
    assert _abi_act(trainer, o.data_ptr(), 0, outs) == 1 and _untouched(outs)         # n = 0
    # clipping off: the bounds are not looked at, not even their order
    off = _run(trainer, o, counter=3, clip_actions=0, action_low=1.0, action_high=-1.0)
    for k in OUT_KEYS:
        assert _biteq(off[k], base[k]), k
    # low == high: every finite env action is that value, act and logp do not move
    flat = _run(trainer, o, counter=3, clip_actions=1, action_low=0.3, action_high=0.3)
    assert (flat["env_act"] == float(np.float32(0.3))).all() and _biteq(flat["act"], base["act"]) and _biteq(flat["logp"], base["logp"])


# ------------------------------------------------------------------------------------------------ 7. scaler blocks at their edges
def test_scaler_blocks_at_their_edges():
    tr = _make_trainer()
    n = 33
    o = _rows(n, seed=90)
    o[:, 3] = 16777216.0 + torch.arange(n, device="cuda").float() * 2.0 - 32.0      # around a mean that is not a float
    blk = tr.state_scaler
    blk[H.OBS + 0] = 1e40                                            # (float)var = inf: standardised 0 for finite o
    blk[H.OBS + 1] = 1e-50                                           # (float)var = 0
    blk[2] = 1e-50                                                   # (float)mean = 0
    blk[3] = 16777217.0                                              # (float)mean = 16777216
    s = tr.standardize(o)
    assert (s[:, 0] == 0).all() and (s[:, 1].abs() == 5.0).all() and s[16, 3] == 0.0 and s[17, 3] > 0.0 > s[15, 3]
    for vblk in ([-1.5, 0.0, 50.0], [-1.5, 1e40, 50.0], [1e39, 4.0, 50.0], [-1.5, 4.0, 50.0]):
        tr.value_scaler.copy_(torch.tensor(vblk, dtype=torch.float64))
        out = _run(tr, o, counter=2)
        mean, val = _reference(tr, o)
        assert _biteq(out["mean"], mean) and torch.isfinite(mean).all() and same_bits_nan_aware(out["val"], val), vblk
        v_raw = _run(tr, o, counter=2, value_scaler=False)["val"]
        assert torch.isfinite(v_raw).all() and (v_raw != 0).all()
        if vblk[1] == 0.0:
            assert (out["val"] == -1.5).all()
        elif vblk[1] == 1e40:
            assert torch.isinf(out["val"]).all() and _biteq(torch.sign(out["val"]), torch.sign(v_raw))
        elif vblk[0] == 1e39:
            assert (out["val"] == H.INF).all()
        else:
            assert torch.isfinite(out["val"]).all()


# ------------------------------------------------------------------------------------ 8. ids, seeds and counters at the top
def _wrap32(x):
    return (x + 2 ** 31) % 2 ** 32 - 2 ** 31


@pytest.mark.parametrize("offset", H.WRAP_OFFSETS)
def test_ids_seeds_and_counters_at_the_top_of_their_ranges(trainer, offset):
    n = 33
    o = _rows(n, seed=100)
    split = 2 ** 31 - offset                                         # the first row whose id is 2**31
    assert 0 < split < n
    seen = []
    for counter in H.TOP_COUNTERS:
        kw = dict(counter=counter, seed_lo=0xFFFFFFFF, seed_hi=0xFFFFFFFF)
        out = _run(trainer, o, env_id_offset=offset, **kw)
        H.check_sampling(out, n, H.LS_CLAMPED, f"offset {offset:#x} counter {counter:#x}", counter=counter, seed=H.TOP_SEED, offset=offset)
        lo = _run(trainer, o[:split].contiguous(), env_id_offset=offset, **kw)
        hi = _run(trainer, o[split:].contiguous(), env_id_offset=_wrap32(offset + split), **kw)      # id 2**31 as the int32 field holds it
        for k in OUT_KEYS:
            assert _biteq(out[k], torch.cat([lo[k], hi[k]])), (counter, k)
        seen.append(out["eps"])
    assert (seen[0] != seen[1]).all() and (seen[1] != seen[2]).all() and (seen[0] != seen[2]).all()


# ------------------------------------------------------------------------------------------------------------ 9. side stream
def test_side_stream(trainer):
    from isaac_rover_orbit_amd import lift_rollout as LR
    n, T = 33, 2
    src = _rows(n, seed=110)
    g = torch.Generator(device="cuda").manual_seed(5)
    rew = torch.randn(n, device="cuda", generator=g)
    term, trunc = torch.rand(n, device="cuda", generator=g) < 0.3, torch.rand(n, device="cuda", generator=g) < 0.3
    log = torch.rand(16, device="cuda", generator=g)
    log[8] = 2.0

    def drive(col, rows):
        ea = col.act(1, rows).clone()
        col.record(1, rew, term, trunc, log)
        return ea, col.last_value(rows).clone()
    ref = LR.LiftRolloutCollector(trainer, n, T, seed=6)
    ref_ea, ref_v = drive(ref, src)
    torch.cuda.synchronize()
    col = LR.LiftRolloutCollector(trainer, n, T, seed=6)
    bufs = (col.obs, col.actions, col.mean, col.logp, col.val, col.rew, col.done, col._env_act, col._last_val)
    filler = torch.zeros(1 << 24, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    for _ in range(8):     # the default stream: a long-running fill, then fills of the collector's own output buffers
        filler.add_(1.0)
    for buf in bufs:
        buf.fill_(FILL)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(4):
            filler.add_(1.0)                 # work queued on s in front of the rows
        rows = src.clone()                   # the rows exist only once s has come this far
        ea, v = drive(col, rows)
        s.synchronize()
    assert _biteq(ea, ref_ea) and _biteq(v, ref_v)
    for name in ("obs", "actions", "mean", "logp", "val", "rew", "done"):
        a, b = getattr(col, name), getattr(ref, name)
        assert _biteq(a[1], b[1]), name
        assert (a[0] == FILL).all(), name                            # slot 0: what the default stream wrote before
    assert _biteq(col.ep_sum, ref.ep_sum) and _biteq(col.ep_count, ref.ep_count) and float(col.ep_count) == 2.0
    torch.cuda.synchronize()
    assert float(filler[0]) == 12.0


# ---------------------------------------------------------------------------------------------------------- 10. record kernel
def _record_buffers(n):
    rew = torch.full((n + 2 * GUARD,), FILL, device="cuda")
    done = torch.full((n + 2 * GUARD,), FILL, device="cuda")
    ep = torch.full((8 + 2 * GUARD,), FILL, device="cuda")
    return rew, done, ep


@pytest.mark.parametrize("n", H.RECORD_NS)
def test_record_bytes_non_finite_rewards_and_the_tally(n):
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd import lift_rollout as LR
    mid = slice(GUARD, GUARD + n)
    for seed, scale in enumerate(H.RECORD_SCALES + (1.0,)):
        rew, term, trunc = H.record_inputs(n, seed)
        want_r, want_d = H.expected_record(rew, term, trunc, scale)
        for flags in ((term, trunc), (term != 0, trunc != 0)):
            spec = LR.TorchLiftRollout(None, None, torch.zeros(8), None, None, n, 1, reward_scale=scale)
            spec.record(0, rew, flags[0], flags[1])
            rbuf, dbuf, _ = _record_buffers(n)
            LR.lift_rollout_record(rew.cuda(), flags[0].cuda(), flags[1].cuda(), float(np.float32(scale)), rbuf[mid], dbuf[mid])
            torch.cuda.synchronize()
            # bitwise; a NaN product (NaN * x, inf * 0) is compared as a position: its payload is the host's or the device's default
            assert same_bits_nan_aware(rbuf[mid].cpu(), spec.rew[0]) and same_bits_nan_aware(spec.rew[0], want_r), (scale, flags[0].dtype)
            assert _biteq(dbuf[mid].cpu(), spec.done[0]) and _biteq(spec.done[0], want_d), (scale, flags[0].dtype)
            for buf in (rbuf, dbuf):
                assert (buf[:GUARD] == FILL).all() and (buf[GUARD + n:] == FILL).all()
            if scale == 1.0:
                assert _biteq(rbuf[mid].cpu(), rew)                   # times one: every bit, NaN payloads and -0.0 included
    # the tally: log[8] = -1, 0, NaN move nothing; log[8] = 3 with a NaN in log[2] poisons ep_sum[2] only
    spec = LR.TorchLiftRollout(None, None, torch.zeros(8), None, None, n, 1)
    rbuf, dbuf, ep = _record_buffers(n)
    ep_sum, ep_count = ep[GUARD:GUARD + 8], torch.zeros((), device="cuda")
    ep_sum.zero_()
    args = (rew.cuda(), term.cuda(), trunc.cuda(), 1.0, rbuf[mid], dbuf[mid])
    for log in [H.record_log(2.0, 1)] + [H.record_log(k, 2) for k in H.STILL_KS] + [H.record_log(3.0, 3, nan_at=2)]:
        before = (ep_sum.clone(), ep_count.clone())
        want_s, want_c = H.expected_tally(spec.ep_sum, spec.ep_count, log)
        spec.record(0, rew, term, trunc, log)
        LR.lift_rollout_record(*args, log.cuda(), ep_sum, ep_count)
        torch.cuda.synchronize()
        assert same_bits_nan_aware(ep_sum.cpu(), spec.ep_sum) and _biteq(ep_count.cpu(), spec.ep_count), log[8]
        assert same_bits_nan_aware(spec.ep_sum, want_s) and _biteq(spec.ep_count, want_c), log[8]
        if not float(log[8]) > 0:
            assert _biteq(ep_sum, before[0]) and _biteq(ep_count, before[1]) and (ep_sum != 0).all(), log[8]
    assert torch.isnan(ep_sum[2]) and torch.isfinite(ep_sum[[0, 1, 3, 4, 5, 6, 7]]).all() and float(ep_count) == 5.0
    assert (ep[:GUARD] == FILL).all() and (ep[GUARD + 8:] == FILL).all()
    snap = (rbuf.clone(), dbuf.clone(), ep.clone())
    with pytest.raises(ValueError):                                   # the wrapper: a log vector needs ep_sum and ep_count
        LR.lift_rollout_record(*args, log.cuda())
    lib = _lib.load()
    rc = lib.rover_lift_rollout_record(args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), n, C.c_float(1.0), log.cuda().data_ptr(),
                                       rbuf[mid].data_ptr(), dbuf[mid].data_ptr(), None, ep_count.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 1                                                    # ROVER_ERR_INVALID, nothing launched
    for a, b in zip((rbuf, dbuf, ep), snap):
        assert same_bits_nan_aware(a, b)


# ------------------------------------------------------------------------------------------------------- 11. collector slots
def test_collector_at_a_ragged_misaligned_shape(trainer):
    from isaac_rover_orbit_amd import lift_rollout as LR
    n, T, off = 17, 3, 2 ** 31 - 10                                  # row 10 has id 2**31
    seed = (5 << 32) | 9
    col = LR.LiftRolloutCollector(trainer, n, T, seed=seed, env_id_offset=off)
    slots = (col.obs, col.actions, col.mean, col.logp, col.val)
    for buf in slots:
        buf.fill_(FILL)
    assert col.logp[1].data_ptr() % 16 != 0 and col.val[1].data_ptr() % 16 != 0       # a slot of 17 floats starts 4 bytes off
    rows = [_rows(n, seed=120 + t) for t in range(T)]
    fresh = None
    for step, t in enumerate((2, 0, 1)):
        if step == 2:     # the checkpoint after two steps resumes the stream in a fresh collector
            fresh = LR.LiftRolloutCollector(trainer, n, T)
            fresh.load_state_dict(col.state_dict())
            assert fresh.state_dict() == {"seed": seed, "counter": 2, "env_id_offset": off}
        for buf in slots:
            for u in (2, 0, 1)[step:]:
                assert (buf[u] == FILL).all()                         # the slots not written yet
        ea = col.act(t, rows[t]).clone()
        ref = _run(trainer, rows[t], counter=step, seed_lo=9, seed_hi=5, env_id_offset=off)
        for k, buf in (("obs", col.obs), ("mean", col.mean), ("act", col.actions), ("logp", col.logp)):
            assert _biteq(buf[t], ref[k]), (t, k)
        assert _biteq(col.val[t], ref["val"][:, 0]) and _biteq(ea, ref["act"]) and col.counter == step + 1
        H.check_sampling(ref, n, H.LS_CLAMPED, f"collector step {step}", counter=step, seed=seed, offset=off)
    assert _biteq(fresh.act(1, rows[1]), ea) and _biteq(fresh.logp[1], col.logp[1]) and fresh.counter == 3
    snap = [buf.clone() for buf in slots]
    v = col.last_value(rows[1])
    torch.cuda.synchronize()
    assert col.counter == 3 and _biteq(v, col.val[1])
    for buf, was in zip(slots, snap):
        assert _biteq(buf, was)
