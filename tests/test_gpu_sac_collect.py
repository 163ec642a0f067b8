"""The fused SAC transition collector on the MI355X (include/rover_sac_collect.h, isaac_rover_orbit_amd.sac_collect) against its
specification.  Random packed weights (tests/helpers.py, scale 3) and synthetic rows (tests/rollout_helpers.py), at most 257 rows per
case; every output is filled with a sentinel and sits between 16 guard elements that are checked after each launch.  Comparisons
are on the bits unless a bound is named.

  * mean_out against the tanh RoverNet forward (rover_policy_forward) at n in {1, 15, 16, 17, 33}, on a ring slot 4 bytes off a
    16-byte boundary and over 1, 3, 5 weight replicas; against float64 torch within 2e-5
  * sigma_out against cephes_expf(clamp(log_std)); eps_out against the float64 Box-Muller under the SAC tag within EPS_TOL at the
    top of the counter, seed and id ranges
  * act_out, env_act_out, logp_out against head() on the kernel's own mean_out and eps_out, both clamps hit
  * NaN in log_std or in the mean stays NaN; MEAN and RANDOM leave what they do not write at the sentinel
  * record against rover_td3_collect_record and rover_td3_smooth_draw
  * SACCollector against TorchSACCollector over two wraps of the ring, then one FusedSAC.update on its memory
  * shards, the checkpoint, a side stream
"""
import numpy as np
import pytest
import torch

from helpers import random_policy_weights, torch_policy_reference
from rollout_helpers import _biteq, synthetic_rows

pytestmark = pytest.mark.gpu

# tests/test_gpu_rollout.py: the largest |eps_kernel - eps_float64| measured on the MI355X for this Box-Muller text is 5.117e-07
# (2**19 draws); the bound is four times that.  The test prints its own maximum before it asserts.
EPS_RECORDED_MAX = 5.117e-07
EPS_TOL = 4.0 * EPS_RECORDED_MAX
MEAN_TOL = 2e-5        # tests/test_gpu_td3_collect_edges.py: this network, random_policy_weights(scale=3.0), against float64 torch
WEIGHT_SEED = 21
SENTINEL = 777.0
GUARD = 16
LOG_STDS = [(0.5, -1.0), (2.5, -25.0), (2.0, -20.0)]
# the clamp condition of test_act_and_logp_are_the_head_on_the_bits, met by the CPU spec alone (torch_policy_reference for the mean,
# the float64 draws) at these seeds: 14 elements at +1, 19 at -1, 33 of 66 inside, no x within 5e-3 of a bound
HEAD_CASE = dict(rows_seed=0, seed=(5 << 32) | 9, env_id_offset=11, counter=5)
F = np.float32


def _actor(seed=WEIGHT_SEED, bias=None):
    from isaac_rover_orbit_amd.policy import RoverNet
    ws, bs = random_policy_weights(seed=seed, out_dim=2, scale=3.0)
    if bias is not None:
        bs[5] = np.asarray(bias, dtype=F)
    return RoverNet(ws, bs, n_enc=2, final_act="tanh")


@pytest.fixture(scope="module")
def actor():
    return _actor()


@pytest.fixture(scope="module")
def clean():
    """(112, 965) sanitised rows, as a ring slot holds them; the first 33 are synthetic_rows(33, seed=0)'s."""
    rows = torch.cat([synthetic_rows(33, seed=0), synthetic_rows(79, seed=7)])
    return torch.nan_to_num(rows, nan=0.0, neginf=0.0).contiguous()


@pytest.fixture(scope="module")
def ref64(clean):
    """The float64 tanh mean on ``clean``, computed once."""
    ws, bs = random_policy_weights(seed=WEIGHT_SEED, out_dim=2, scale=3.0)
    return torch_policy_reference([w.astype(np.float64) for w in ws], [b.astype(np.float64) for b in bs],
                                  clean.cpu().numpy().astype(np.float64), final_tanh=True)


def _guarded(numel, dtype=torch.float32, offset=0):
    """A sentinel-filled buffer with GUARD elements on either side of a view of ``numel`` elements, the view ``offset`` elements off a
    16-byte boundary for 4-byte types."""
    fill = {torch.float32: SENTINEL, torch.int32: -7, torch.int64: -7, torch.uint8: 99}[dtype]
    buf = torch.full((GUARD + offset + numel + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD + offset:GUARD + offset + numel], fill


def _guards_intact(buf, view, fill):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == fill).all()) and bool((buf[lo + view.numel():] == fill).all())


def _hp(**kw):
    from isaac_rover_orbit_amd import sac_collect as SC
    hp = SC.default_hparams()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def _ls(pair):
    return torch.tensor(pair, dtype=torch.float32, device="cuda")


def _act(actor, log_std, rows, counter=0, **hp):
    """One act launch into sentinel-filled, guarded outputs; returns mean, act, env_act, eps (n, 2), logp (n,), sigma (2,)."""
    from isaac_rover_orbit_amd import sac_collect as SC
    n = rows.shape[0]
    bufs = {k: _guarded(numel) for k, numel in (("mean", 2 * n), ("act", 2 * n), ("env_act", 2 * n), ("eps", 2 * n), ("logp", n), ("sigma", 2))}
    o = {k: v[1] if k in ("logp", "sigma") else v[1].view(n, 2) for k, v in bufs.items()}
    SC.collect_act(actor, log_std, rows, counter, _hp(**hp), o["act"], o["env_act"], mean_out=o["mean"], eps_out=o["eps"],
                   logp_out=o["logp"], sigma_out=o["sigma"])
    torch.cuda.synchronize()
    for k, (buf, view, fill) in bufs.items():
        assert _guards_intact(buf, view, fill), k
    return o


def _untouched(t):
    return bool((t == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------ mean
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_mean_against_policy_forward(actor, clean, ref64, n):
    rows = clean[:n].contiguous()
    want = actor(rows)
    o = _act(actor, _ls((0.5, -1.0)), rows, counter=3)
    assert torch.isfinite(want).all() and _biteq(o["mean"], want)
    d = float(np.abs(o["mean"].cpu().numpy().astype(np.float64) - ref64[:n]).max())
    print(f"n={n}: max |mean - float64| = {d:.3e} (bound {MEAN_TOL:.0e})")
    assert d <= MEAN_TOL
    assert _biteq(o["act"], o["env_act"]) and float(o["act"].abs().max()) <= 1.0 and not _untouched(o["eps"]) and not _untouched(o["logp"])
    # the optional outputs are optional
    from isaac_rover_orbit_amd import sac_collect as SC
    a, e = torch.full((n, 2), SENTINEL, device="cuda"), torch.full((n, 2), SENTINEL, device="cuda")
    SC.collect_act(actor, _ls((0.5, -1.0)), rows, 3, _hp(), a, e)
    torch.cuda.synchronize()
    assert _biteq(a, o["act"]) and _biteq(e, o["env_act"])


def test_mean_on_a_ring_slot_off_alignment(actor, clean):
    """Slot 1 of an n = 17 ring starts 17 * 965 * 4 bytes in: 4 bytes off a 16-byte boundary, the scalar staging path."""
    ring = torch.zeros(2, 17, 965, device="cuda")
    ring[1] = clean[:17]
    assert ring.data_ptr() % 16 == 0 and ring[1].data_ptr() % 16 == 4 and ring[1].is_contiguous()
    aligned = _act(actor, _ls((0.5, -1.0)), clean[:17].contiguous(), counter=2)
    o = _act(actor, _ls((0.5, -1.0)), ring[1], counter=2)
    for k in o:
        assert _biteq(o[k], aligned[k]), k
    assert _biteq(o["mean"], actor(clean[:17].contiguous()))


def test_number_of_weight_replicas(actor, clean):
    """Seven workgroups (n = 112) over k = 1, 3, 5 replicas; one more replica-sized block of NaN follows the last replica."""
    from isaac_rover_orbit_amd.policy import RoverNet
    pf = actor.packed.numel() // actor.n_copies
    results = []
    for k in (1, 3, 5):
        buf = torch.full(((k + 1) * pf,), float("nan"), dtype=torch.float32, device="cuda")
        buf[:k * pf] = actor.packed[:pf].repeat(k)
        net = RoverNet.from_packed(actor.desc, buf[:k * pf], k)
        o = _act(net, _ls((0.5, -1.0)), clean, counter=2)
        assert o["mean"].shape == (112, 2)
        for key in o:
            assert torch.isfinite(o[key]).all(), (k, key)
        results.append(o)
    for o in results[1:]:
        for key in o:
            assert _biteq(o[key], results[0][key]), key
    assert _biteq(results[0]["mean"], actor(clean))


# --------------------------------------------------------------------------------------------------------------- sigma and eps
@pytest.mark.parametrize("log_std", LOG_STDS)
def test_sigma_is_the_cephes_exp_of_the_clamped_log_std(actor, clean, log_std):
    from isaac_rover_orbit_amd import sac_collect as SC
    o = _act(actor, _ls(log_std), clean[:17].contiguous())
    want = SC.cephes_expf(SC.tclamp(np.asarray(log_std, dtype=F), -20.0, 2.0))
    assert np.array_equal(o["sigma"].cpu().numpy().view(np.int32), want.view(np.int32)), (o["sigma"], want)
    assert abs(float(want[0]) / np.exp(min(log_std[0], 2.0)) - 1.0) <= 2.0 ** -22


def test_eps_against_the_float64_spec(actor, clean):
    from isaac_rover_orbit_amd import rollout as R
    from isaac_rover_orbit_amd import sac_collect as SC
    rows, top = clean[:33].contiguous(), 2 ** 31 - 2 - 32
    seed = 2 ** 64 - 1
    worst, seen = 0.0, []
    for off in (11, top):
        for counter in (0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1):
            eps = _act(actor, _ls((0.5, -1.0)), rows, counter=counter, seed_lo=0xFFFFFFFF, seed_hi=0xFFFFFFFF, env_id_offset=off)["eps"]
            ids = off + np.arange(33)
            ref = R.standard_normals(seed, ids, counter, 2, tag=SC.ACTION_TAG)
            worst = max(worst, float(np.abs(eps.cpu().numpy().astype(np.float64) - ref).max()))
            seen.append(eps)
    assert ids[-1] == 2 ** 31 - 2
    print(f"max |eps_kernel - eps_float64| over {8 * 66} draws (seed 2**64 - 1, ids up to 2**31 - 2) = {worst:.3e}; bound {EPS_TOL:.3e}")
    assert worst <= EPS_TOL
    assert all(not _biteq(seen[i], seen[j]) for i in range(8) for j in range(i))
    other = R.standard_normals(seed, ids, 2 ** 64 - 1, 2)                               # the rollout collector's stream: another one
    assert np.abs(seen[-1].cpu().numpy() - other).max() > 0.1


# --------------------------------------------------------------------------------------------------------------------- the head
@pytest.mark.parametrize("log_std", LOG_STDS[:2])
def test_act_and_logp_are_the_head_on_the_bits(actor, log_std):
    from isaac_rover_orbit_amd import sac_collect as SC
    c = HEAD_CASE
    rows = torch.nan_to_num(synthetic_rows(33, seed=c["rows_seed"]), nan=0.0, neginf=0.0).contiguous()
    o = _act(actor, _ls(log_std), rows, counter=c["counter"], seed_lo=c["seed"] & 0xFFFFFFFF, seed_hi=c["seed"] >> 32,
             env_id_offset=c["env_id_offset"])
    u, logp, sigma = SC.head(o["mean"].cpu().numpy(), log_std, o["eps"].cpu().numpy())
    assert _biteq(o["act"].cpu(), torch.from_numpy(u)) and _biteq(o["env_act"], o["act"])
    assert _biteq(o["logp"].cpu(), torch.from_numpy(logp)) and np.isfinite(logp).all()
    assert _biteq(o["sigma"].cpu(), torch.from_numpy(sigma)) and _biteq(o["mean"], actor(rows))
    if log_std == (0.5, -1.0):
        # the CPU spec alone meets the condition at these seeds ...
        ws, bs = random_policy_weights(seed=WEIGHT_SEED, out_dim=2, scale=3.0)
        mu_cpu = torch_policy_reference(ws, bs, rows.cpu().numpy(), final_tanh=True)
        eps_cpu = SC.action_normals(c["seed"], c["env_id_offset"] + np.arange(33), c["counter"]).astype(F)
        u_cpu = SC.head(mu_cpu, log_std, eps_cpu)[0]
        for name, v in (("spec", u_cpu), ("kernel", u)):
            hi, lo, inside = int((v == 1).sum()), int((v == -1).sum()), int((np.abs(v) < 1).sum())
            print(f"{name}: {hi} at +1, {lo} at -1, {inside} of {v.size} inside")
            assert hi >= 1 and lo >= 1 and 4 * inside >= v.size and hi + lo + inside == v.size
        assert np.array_equal(np.abs(u_cpu) == 1, np.abs(u) == 1)                       # ... and the kernel clamps the same elements
    else:
        assert np.array_equal(sigma, SC.cephes_expf(np.array([2.0, -20.0], F)))


def test_nan_in_log_std_or_in_the_mean_stays_nan(actor, clean):
    rows = clean[:33].contiguous()
    good = _act(actor, _ls((0.5, -1.0)), rows, counter=4)
    o = _act(actor, _ls((float("nan"), -1.0)), rows, counter=4)                         # column 0 is NaN, column 1 is not touched
    assert torch.isnan(o["act"][:, 0]).all() and torch.isnan(o["env_act"][:, 0]).all() and torch.isnan(o["sigma"][0])
    assert _biteq(o["act"][:, 1], good["act"][:, 1]) and _biteq(o["env_act"][:, 1], good["act"][:, 1])
    assert _biteq(o["mean"], good["mean"]) and _biteq(o["eps"], good["eps"]) and torch.isnan(o["logp"]).all()
    ws, bs = random_policy_weights(seed=WEIGHT_SEED, out_dim=2, scale=3.0)
    nan_net = _actor(bias=[float("nan"), float(bs[5][1])])                              # the mean's column 0 is NaN
    for mode in (0, 1):                                                                 # SAMPLE and MEAN
        o = _act(nan_net, _ls((0.5, -1.0)), rows, counter=4, mode=mode)
        assert torch.isnan(o["mean"][:, 0]).all() and torch.isnan(o["act"][:, 0]).all() and torch.isnan(o["env_act"][:, 0]).all()
        assert not (o["act"][:, 0] == -1.0).any()
        assert _biteq(o["mean"][:, 1], good["mean"][:, 1]) and torch.isfinite(o["act"][:, 1]).all()
        if mode == 0:
            assert _biteq(o["act"][:, 1], good["act"][:, 1])


# -------------------------------------------------------------------------------------------------------------------- the modes
def test_mean_mode(actor, clean):
    from isaac_rover_orbit_amd import sac_collect as SC
    rows = clean[:33].contiguous()
    o = _act(actor, _ls((0.5, -1.0)), rows, counter=4, mode=SC.MEAN)
    want = actor(rows)
    assert _biteq(o["mean"], want) and _biteq(o["act"], want) and _biteq(o["env_act"], want)
    assert _untouched(o["eps"]) and _untouched(o["logp"]) and _untouched(o["sigma"])
    a, e = torch.full((33, 2), SENTINEL, device="cuda"), torch.full((33, 2), SENTINEL, device="cuda")
    SC.collect_act(actor, None, rows, 4, _hp(mode=SC.MEAN), a, e)                       # log_std is not read
    torch.cuda.synchronize()
    assert _biteq(a, want) and _biteq(e, want)


@pytest.mark.parametrize("n", [1, 33, 257])
def test_random_mode(actor, n):
    from isaac_rover_orbit_amd import sac_collect as SC
    from isaac_rover_orbit_amd.policy import RoverNet
    rows = torch.nan_to_num(synthetic_rows(n, seed=5), nan=0.0, neginf=0.0).contiguous()
    seed, counter, off = (3 << 32) | 42, (1 << 32) | 7, 2 ** 31 - 2 - (n - 1)
    kw = dict(counter=counter, mode=SC.RANDOM, seed_lo=seed & 0xFFFFFFFF, seed_hi=seed >> 32, env_id_offset=off)
    o = _act(actor, _ls((0.5, -1.0)), rows, **kw)
    want = torch.from_numpy(SC.random_actions(seed, off + np.arange(n), counter))
    assert _biteq(o["act"].cpu(), want) and _biteq(o["env_act"].cpu(), want) and float(o["act"].abs().max()) < 1.0
    for k in ("mean", "eps", "logp", "sigma"):
        assert _untouched(o[k]), k
    poisoned = RoverNet.from_packed(actor.desc, torch.full_like(actor.packed, float("nan")), actor.n_copies)
    p = _act(poisoned, _ls((float("nan"), float("nan"))), rows, **kw)                  # neither the weights nor log_std are read
    for k in o:
        assert _biteq(p[k], o[k]), k


# --------------------------------------------------------------------------------------------------------------------- record
def _record_inputs(n):
    g = torch.Generator(device="cuda").manual_seed(n)
    raw = synthetic_rows(n, seed=3)
    raw[0, 5], raw[n - 1, 964] = float("nan"), float("inf")
    rew = torch.randn(n, device="cuda", generator=g)
    rew[(n - 1) // 2] = float("nan")
    term = torch.tensor([0, 1, 2, 255], dtype=torch.uint8, device="cuda").repeat(n // 4 + 1)[:n].contiguous()
    return raw, rew, term


@pytest.mark.parametrize("n,B", [(1, 1), (1, 257), (255, 1), (257, 256)])
def test_record_is_the_td3_record_and_the_smooth_draw(n, B):
    from isaac_rover_orbit_amd import sac_collect as SC
    from isaac_rover_orbit_amd import td3_collect as TC
    from isaac_rover_orbit_amd import td3_explore as TX
    raw0, rew, term = _record_inputs(n)
    seed = (3 << 32) | 42
    thp = TC.default_hparams()
    thp.seed_lo, thp.seed_hi = seed & 0xFFFFFFFF, seed >> 32
    shp = _hp(seed_lo=seed & 0xFFFFFFFF, seed_hi=seed >> 32)
    for src_off in (0, 1):
        src_buf, src, _ = _guarded(n * 965, offset=src_off)
        src.copy_(raw0.reshape(-1))
        raw = src.view(n, 965)
        for dst_off in (0, 1):
            for mem_rows, counter in ((1, 0), (3, (1 << 32) | 7), (2 ** 25 + 1, 2 ** 64 - 1)):
                outs = []
                for fn, hp in ((TC.collect_record, thp), (SC.collect_record, shp)):
                    b = dict(slot=_guarded(n * 965, offset=dst_off), rew=_guarded(n, offset=1), term=_guarded(n, torch.uint8),
                             pos=_guarded(1, torch.int32), idx=_guarded(B, torch.int64))
                    assert raw.data_ptr() % 16 == 4 * src_off and b["slot"][1].data_ptr() % 16 == 4 * dst_off
                    fn(raw, b["slot"][1].view(n, 965), hp, counter, rew=rew, terminated=term, rew_out=b["rew"][1], term_out=b["term"][1],
                       ring_pos_entry=b["pos"][1], ring_pos_value=5, idx_out=b["idx"][1], mem_rows=mem_rows)
                    torch.cuda.synchronize()
                    for k, (buf, view, fill) in b.items():
                        assert _guards_intact(buf, view, fill), k
                    outs.append(b)
                t, s = outs
                assert _biteq(s["slot"][1], t["slot"][1]) and _biteq(s["rew"][1], t["rew"][1]) and torch.equal(s["term"][1], t["term"][1])
                assert torch.equal(s["pos"][1], t["pos"][1]) and int(s["pos"][1]) == 5 and torch.equal(s["idx"][1], t["idx"][1])
                assert _biteq(s["slot"][1].view(n, 965), torch.nan_to_num(raw, nan=0.0, neginf=0.0))
                assert s["idx"][1].tolist() == TC.sample_indices(seed, counter, B, mem_rows).tolist()
    # with eps_out: rover_td3_smooth_draw at std = 1 and A = 4, beside unchanged indices
    raw = raw0
    for counter in (0, 2 ** 32 + 7):
        want = TX.smooth_draw(seed, counter, 1.0, torch.full((B, 4), SENTINEL, device="cuda"))
        b = dict(slot=_guarded(n * 965), idx=_guarded(B, torch.int64), eps=_guarded(4 * B))
        assert b["eps"][1].data_ptr() % 16 == 0
        SC.collect_record(raw, b["slot"][1].view(n, 965), shp, counter, idx_out=b["idx"][1], mem_rows=1000, eps_out=b["eps"][1].view(B, 4))
        torch.cuda.synchronize()
        for k, (buf, view, fill) in b.items():
            assert _guards_intact(buf, view, fill), k
        assert _biteq(b["eps"][1].view(B, 4), want) and not _untouched(want)
        assert b["idx"][1].tolist() == TC.sample_indices(seed, counter, B, 1000).tolist()
        assert _biteq(b["slot"][1].view(n, 965), torch.nan_to_num(raw, nan=0.0, neginf=0.0))
        d = np.abs(want.cpu().numpy().astype(np.float64) - TX.smooth_normals(seed, counter, B, 4)).max()
        assert d <= EPS_TOL
        only = _guarded(4 * B)                                                          # the draws without indices
        SC.collect_record(raw, b["slot"][1].view(n, 965), shp, counter, eps_out=only[1].view(B, 4))
        torch.cuda.synchronize()
        assert _biteq(only[1].view(B, 4), want) and _guards_intact(*only)
    # the begin form: every record pointer NULL, only the rows go in
    slot = _guarded(n * 965)
    SC.collect_record(raw, slot[1].view(n, 965), _hp())
    torch.cuda.synchronize()
    assert _biteq(slot[1].view(n, 965), torch.nan_to_num(raw, nan=0.0, neginf=0.0)) and _guards_intact(*slot)
    with pytest.raises(Exception, match="aligned"):
        SC.collect_record(raw, slot[1].view(n, 965), shp, 0, eps_out=_guarded(4 * B, offset=1)[1].view(B, 4))


# ------------------------------------------------------------------------------------------------------------- the collector
def _step_inputs(n, t):
    raw = synthetic_rows(n, seed=10 + t)
    raw[t % n, 7 + t] = float("nan")
    raw[(t + 3) % n, 964] = float("inf")
    g = torch.Generator(device="cuda").manual_seed(50 + t)
    return raw, torch.randn(n, device="cuda", generator=g), torch.rand(n, device="cuda", generator=g) < 0.3


@pytest.fixture(scope="module")
def fused():
    from isaac_rover_orbit_amd.sac import FusedSAC
    from sac_helpers import nets
    return FusedSAC(*(m.state_dict() for m in nets(seed=3, log_std=(-0.5, -1.5))))


def test_collector_against_the_spec_and_into_the_update(fused):
    from isaac_rover_orbit_amd import sac_collect as SC
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    n, M, steps, B = 17, 2, 5, 64
    mem, ref = ReplayMemory(M, n, device="cuda"), ReplayMemory(M, n, device="cpu")
    kw = dict(seed=(7 << 32) | 5, env_id_offset=100, random_timesteps=1)
    col = SC.SACCollector(fused.actor, fused.log_std, mem, **kw)
    spec = SC.TorchSACCollector(lambda o: fused.actor(o.cuda().contiguous()).cpu(), fused.log_std, ref, **kw)
    raw0 = _step_inputs(n, 99)[0]
    col.begin(raw0)
    spec.begin({"policy": raw0.cpu()})
    f = dict(dtype=torch.float32, device="cuda")
    mean, eps, logp, sigma = torch.empty(n, 2, **f), torch.empty(n, 2, **f), torch.empty(n, **f), torch.empty(2, **f)
    for t in range(steps):
        k = mem.memory_index
        a = col.act(t, mean_out=mean, eps_out=eps, logp_out=logp, sigma_out=sigma)
        torch.cuda.synchronize()
        b = spec.act(t, eps=eps)                                                        # the spec is given the kernel's own draws
        assert _biteq(a, mem.actions[k]) and _biteq(a.cpu(), b), t
        if t >= 1:
            assert _biteq(mean, fused.actor(mem.obs[mem.cursor])) and _biteq(logp.cpu(), spec.last["logp"])
            assert _biteq(sigma.cpu(), spec.last["sigma"]) and _biteq(mean.cpu(), spec.last["mean"])
        raw, rew, term = _step_inputs(n, t)
        i, e = col.record(raw, rew, term, B)
        j, e_spec = spec.record(raw.cpu(), rew.cpu(), term.cpu(), B)
        assert i.dtype == torch.int64 and torch.equal(i.cpu(), j) and int(i.max()) < len(mem) and int(i.min()) >= 0
        assert e.shape == (B, 4) and float((e.cpu() - e_spec).abs().max()) <= EPS_TOL
        for name in ("obs", "actions", "rewards", "terminated", "ring_pos"):
            x, y = getattr(mem, name).cpu(), getattr(ref, name)
            assert torch.equal(x, y) and (x.dtype == torch.bool or _biteq(x, y)), (t, name)
        assert len(mem) == len(ref) == min(t + 1, M) * n
        assert (mem.memory_index, mem.filled, mem.cursor) == (ref.memory_index, ref.filled, ref.cursor)
        assert col.state_dict() == spec.state_dict() == {"seed": (7 << 32) | 5, "counter": 2 * (t + 1), "env_id_offset": 100}
    assert mem.filled and mem._last_next is None and torch.isfinite(mem.obs).all()
    before = fused.log_std.clone()
    fused.update(mem, i, e)
    st = fused.stats()
    assert st["bad_index"] == 0 and np.isfinite(st["critic_loss"]) and np.isfinite(st["policy_loss"])
    assert (st["critic_step"], st["actor_step"]) == (1, 1) and not torch.equal(before, fused.log_std)
    # held by reference: the next act sees the updated actor and log_std
    col.act(steps, mean_out=mean, sigma_out=sigma)
    torch.cuda.synchronize()
    assert _biteq(mean, fused.actor(mem.obs[mem.cursor]))
    want = SC.cephes_expf(SC.tclamp(fused.log_std.cpu().numpy(), -20.0, 2.0))
    assert _biteq(sigma.cpu(), torch.from_numpy(want)) and not np.array_equal(want, SC.cephes_expf(before.cpu().numpy()))
    # arguments are validated as TD3Collector validates them
    raw, rew, term = _step_inputs(n, 0)
    for bad in ((raw[:5], rew, term), (raw.cpu(), rew, term), (raw, rew.double(), term), (raw, rew, term.float()), (raw, rew[:3], term)):
        with pytest.raises(ValueError):
            col.record(*bad)
    with pytest.raises(ValueError):
        col.begin(raw.double())
    with pytest.raises(ValueError):
        SC.SACCollector(fused.actor, fused.log_std, ReplayMemory(M, n, device="cuda", act_dim=3))
    with pytest.raises(ValueError):
        SC.SACCollector(fused.actor, fused.log_std.cpu(), mem)


def test_shards_checkpoint_and_a_side_stream(actor, clean):
    from isaac_rover_orbit_amd import sac_collect as SC
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    M, B, seed = 4, 33, (9 << 32) | 5
    log_std = _ls((0.5, -1.0))
    make = lambda n, off: SC.SACCollector(actor, log_std, ReplayMemory(M, n, device="cuda"), seed=seed, env_id_offset=off,   # noqa: E731
                                          random_timesteps=1)
    whole, parts, sl = make(33, 0), [make(16, 0), make(17, 16)], (slice(0, 16), slice(16, 33))
    raw = _step_inputs(33, 99)[0]
    whole.begin(raw)
    for p, s in zip(parts, sl):
        p.begin(raw[s].contiguous())
    acts, batches, saved = [], [], None
    for t in range(5):
        if t == 2:                                                                      # the checkpoint after step 2
            saved = (whole.state_dict(), {k: getattr(whole.memory, k).clone() for k in ("obs", "actions", "rewards", "terminated", "ring_pos")},
                     (whole.memory.cursor, whole.memory.memory_index, whole.memory.filled))
        a = whole.act(t).clone()
        if t < 3:                                                                       # shards of 16 and 17 envs equal the whole
            assert _biteq(a, torch.cat([p.act(t) for p in parts])), t
        raw, rew, term = _step_inputs(33, t)
        i, e = whole.record(raw, rew, term, B)
        if t < 3:
            for p, s in zip(parts, sl):
                pi, pe = p.record(raw[s].contiguous(), rew[s].contiguous(), term[s].contiguous(), B)
                assert _biteq(pe, e)                                                    # the draws do not depend on the shard
            for name in ("obs", "actions", "rewards", "terminated"):
                x, y = getattr(whole.memory, name), torch.cat([getattr(p.memory, name) for p in parts], 1)
                assert torch.equal(x, y) and (x.dtype == torch.bool or _biteq(x, y)), (t, name)
        acts.append(a)
        batches.append((i.clone(), e.clone()))
    assert not _biteq(acts[1], acts[2]) and float(acts[0].abs().max()) < 1.0
    fresh = make(33, 7)
    fresh.load_state_dict(saved[0])
    for k, v in saved[1].items():
        getattr(fresh.memory, k).copy_(v)
    fresh.memory.cursor, fresh.memory.memory_index, fresh.memory.filled = saved[2]
    assert fresh.state_dict() == {"seed": seed, "counter": 4, "env_id_offset": 0}
    for t in (2, 3):                                                                    # ... reproduces steps 3 and 4
        assert _biteq(fresh.act(t), acts[t]), t
        raw, rew, term = _step_inputs(33, t)
        i, e = fresh.record(raw, rew, term, B)
        assert torch.equal(i, batches[t][0]) and _biteq(e, batches[t][1])
    # one act and one record on a side stream
    rows = clean[:33].contiguous()
    want = _act(actor, log_std, rows, counter=6)
    raw = synthetic_rows(33, seed=4)
    slot, idx, eps = torch.zeros(33, 965, device="cuda"), torch.zeros(65, dtype=torch.int64, device="cuda"), torch.zeros(65, 4, device="cuda")
    SC.collect_record(raw, slot, _hp(), 6, idx_out=idx, mem_rows=1000, eps_out=eps)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _act(actor, log_std, rows, counter=6)
        slot2, idx2, eps2 = torch.zeros(33, 965, device="cuda"), torch.zeros(65, dtype=torch.int64, device="cuda"), torch.zeros(65, 4, device="cuda")
        SC.collect_record(raw, slot2, _hp(), 6, idx_out=idx2, mem_rows=1000, eps_out=eps2)
    side.synchronize()
    for k in want:
        assert _biteq(got[k], want[k]), k
    assert _biteq(slot2, slot) and torch.equal(idx2, idx) and _biteq(eps2, eps) and _biteq(slot, torch.nan_to_num(raw, nan=0.0, neginf=0.0))
