"""The fused TD3 transition collector on the MI355X (include/rover_td3_collect.h, isaac_rover_orbit_amd.td3_collect) against its
specification.  Random packed weights (tests/helpers.py) and synthetic rows (tests/rollout_helpers.py), at most 257 rows per case.

  * mean_out BIT-EXACT against rover_policy_forward at n in {1, 15, 16, 17, 33} and on a ring slot 4 bytes off a 16-byte boundary
  * explore = 0: act_out == env_act_out == mean_out on the bits, eps_out untouched
  * eps against the float64 Box-Muller of rollout.standard_normals under the collector's tag: EPS_TOL below, the bound DESIGN 16
    has on record for this Box-Muller text (four times the 5.117e-07 measured there, <= 1e-5)
  * act BIT-EXACT against td3.explore in fp32 torch on the kernel's own mean_out and eps_out, at two pairs of bounds
  * record: nan_to_num on the bits at both alignments, reward / terminated / ring_pos / the indices, guards around every output
  * TD3Collector against TorchTD3Collector over two wraps of the ring, then one FusedTD3.critic_step on its memory
  * the split over two calls, and a side stream
"""
import numpy as np
import pytest
import torch

from helpers import random_policy_weights
from rollout_helpers import _biteq, synthetic_rows

pytestmark = pytest.mark.gpu

# tests/test_gpu_rollout.py: the largest |eps_kernel - eps_float64| measured on the MI355X for this Box-Muller text is 5.117e-07
# (2**19 draws); the bound is four times that.  The maximum over this file's 528 + 4224 draws (pairs 0 .. 7) is printed by the
# test before it asserts; DESIGN 18 records it.
EPS_RECORDED_MAX = 5.117e-07
EPS_TOL = 4.0 * EPS_RECORDED_MAX
assert EPS_TOL <= 1e-5
SENTINEL = 777.0
GUARD = 16


def _actor(A=2, seed=21):
    from isaac_rover_orbit_amd.policy import RoverNet
    ws, bs = random_policy_weights(seed=seed, out_dim=A, scale=3.0)
    return RoverNet(ws, bs, n_enc=2, final_act="none")


@pytest.fixture(scope="module")
def actor():
    return _actor(2)


@pytest.fixture(scope="module")
def clean():
    """(33, 965) sanitised rows, as a ring slot holds them."""
    return torch.nan_to_num(synthetic_rows(33, seed=0), nan=0.0, neginf=0.0).contiguous()


def _hp(**kw):
    from isaac_rover_orbit_amd import td3_collect as TC
    hp = TC.default_hparams()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def _act(actor, rows, counter=0, **hp):
    """One act launch into sentinel-filled outputs; returns mean, act, env_act, eps."""
    from isaac_rover_orbit_amd import td3_collect as TC
    n, A = rows.shape[0], actor.out_dim
    o = {k: torch.full((n, A), SENTINEL, dtype=torch.float32, device="cuda") for k in ("mean", "act", "env_act", "eps")}
    TC.collect_act(actor, rows, counter, _hp(**hp), o["act"], o["env_act"], mean_out=o["mean"], eps_out=o["eps"])
    torch.cuda.synchronize()
    return o


# ------------------------------------------------------------------------------------------------------------------------ act
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_mean_against_policy_forward_and_the_plain_path(actor, clean, n):
    rows = clean[:n].contiguous()
    want = actor(rows)
    o = _act(actor, rows, counter=3)
    assert torch.isfinite(want).all() and _biteq(o["mean"], want)
    assert _biteq(o["act"], want) and _biteq(o["env_act"], want)                       # explore = 0: the output, not clamped
    assert (want.abs() > 1.0).any() or n < 33
    assert (o["eps"] == SENTINEL).all()                                                # ... and no draw
    # mean_out and eps_out are optional
    from isaac_rover_orbit_amd import td3_collect as TC
    a, e = torch.full((n, 2), SENTINEL, device="cuda"), torch.full((n, 2), SENTINEL, device="cuda")
    TC.collect_act(actor, rows, 3, _hp(explore=1, noise_std=0.5), a, e)
    full = _act(actor, rows, counter=3, explore=1, noise_std=0.5)
    assert _biteq(a, full["act"]) and _biteq(e, full["env_act"]) and _biteq(full["mean"], want)


def test_mean_on_a_ring_slot_off_alignment(actor, clean):
    """Slot 1 of an n = 17 ring starts 17 * 965 * 4 bytes in: 4 bytes off a 16-byte boundary, the scalar staging path."""
    ring = torch.zeros(2, 17, 965, device="cuda")
    ring[1] = clean[:17]
    assert ring.data_ptr() % 16 == 0 and ring[1].data_ptr() % 16 == 4 and ring[1].is_contiguous()
    aligned = _act(actor, clean[:17].contiguous())
    o = _act(actor, ring[1])
    for k in ("mean", "act", "env_act"):
        assert _biteq(o[k], aligned[k]), k
    assert _biteq(o["mean"], actor(clean[:17].contiguous()))


@pytest.mark.parametrize("A", [2, 16])
def test_eps_against_the_float64_spec(clean, A):
    from isaac_rover_orbit_amd import rollout as R
    from isaac_rover_orbit_amd import td3_collect as TC
    net = _actor(A)
    worst, biggest = 0.0, 0.0
    for k in (0, 1, 2, 3, 4, 5, 6, 2 ** 32 + 7):
        eps = _act(net, clean, counter=k, explore=1, noise_std=0.1, seed_lo=9, seed_hi=5, env_id_offset=11)["eps"]
        ref = R.standard_normals((5 << 32) | 9, 11 + np.arange(33), k, A, tag=TC.NOISE_TAG)
        d = np.abs(eps.cpu().numpy().astype(np.float64) - ref)
        worst, biggest = max(worst, float(d.max())), max(biggest, float(np.abs(ref).max()))
    print(f"A={A}: max |eps_kernel - eps_float64| over {8 * 33 * A} draws = {worst:.3e} (largest |eps| {biggest:.3f}); bound {EPS_TOL:.3e}")
    assert worst <= EPS_TOL
    other = _act(net, clean, counter=0, explore=1, noise_std=0.1, seed_lo=9, seed_hi=5, env_id_offset=11)["eps"]
    rol = R.standard_normals((5 << 32) | 9, 11 + np.arange(33), 0, A)                  # the rollout collector's stream: another one
    assert np.abs(other.cpu().numpy() - rol).max() > 0.1


@pytest.mark.parametrize("low,high", [(-1.0, 1.0), (-0.25, 0.5)])
def test_act_with_noise_is_td3_explore_on_the_bits(actor, clean, low, high):
    from isaac_rover_orbit_amd.td3 import explore
    std, scale = 0.3, 0.7                                                               # neither is a power of two in fp32
    o = _act(actor, clean, counter=5, explore=1, noise_std=std, noise_scale=scale, action_low=low, action_high=high)
    want = explore(o["mean"], std * o["eps"], scale, low, high)                         # three fp32 operations, then the clamp
    assert _biteq(o["act"], want) and _biteq(o["env_act"], o["act"])
    assert _biteq(o["mean"], actor(clean))
    a = o["act"]
    hit_low, hit_high, inside = a == low, a == high, (a > low) & (a < high)
    print(f"[{low}, {high}]: {int(hit_low.sum())} at low, {int(hit_high.sum())} at high, {int(inside.sum())} inside of {a.numel()}")
    assert hit_low.any() and inside.any() and (hit_low | hit_high | inside).all()
    assert hit_low[:, 1].sum() > hit_low[:, 0].sum()                                    # column 1 clips, column 0 mostly does not
    if high < 1.0:
        assert hit_high.any()
    unclamped = o["mean"] + (std * o["eps"]) * scale
    assert not _biteq(unclamped, a)                                                     # the clamp did something
    zero = _act(actor, clean, counter=5, explore=1, noise_std=0.0, noise_scale=scale, action_low=low, action_high=high)
    assert _biteq(zero["act"], zero["mean"].clamp(low, high))                           # explore = 1 with no noise still clamps


def test_split_over_two_calls(actor, clean):
    kw = dict(counter=4, explore=1, noise_std=0.3, noise_scale=0.9)
    whole = _act(actor, clean, env_id_offset=0, **kw)
    lo = _act(actor, clean[:16].contiguous(), env_id_offset=0, **kw)
    hi = _act(actor, clean[16:].contiguous(), env_id_offset=16, **kw)
    for k in whole:
        assert _biteq(whole[k], torch.cat([lo[k], hi[k]])), k
    again, nxt = _act(actor, clean, **kw), _act(actor, clean, **dict(kw, counter=5))
    assert _biteq(again["eps"], whole["eps"]) and (nxt["eps"] != whole["eps"]).all()


# --------------------------------------------------------------------------------------------------------------------- record
def _guarded(numel, dtype, offset=0):
    """A sentinel-filled buffer with GUARD elements on either side of a view of ``numel`` elements, the view ``offset`` elements off a
    16-byte boundary for 4-byte types."""
    fill = {torch.float32: SENTINEL, torch.int32: -7, torch.int64: -7, torch.uint8: 99}[dtype]
    buf = torch.full((GUARD + offset + numel + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD + offset:GUARD + offset + numel], fill


def _guards_intact(buf, view, fill):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == fill).all()) and bool((buf[lo + view.numel():] == fill).all())


SPECIAL_BITS = [0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00011A2B, 0x80011A2B]   # NaN +/-, signalling
                                                                                      # NaN, +inf, -inf, -0.0, a denormal of each sign


@pytest.mark.parametrize("n", [1, 16, 17])
@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_record_sanitises_on_the_bits(n, src_off, dst_off):
    """The special values at elements 0, 511, 512 and the last (and at 1023, 1024, 4095, 4096, where a thread's next piece and the
    next block begin), every value at every place over the rotations; source and destination 0 and 4 bytes off alignment."""
    from isaac_rover_orbit_amd import td3_collect as TC
    total = n * 965
    base = synthetic_rows(n, seed=2).reshape(-1)
    places = [p for p in (0, 511, 512, 1023, 1024, 4095, 4096, total - 1) if p < total]
    for rot in range(len(SPECIAL_BITS)):
        src_buf, src, _ = _guarded(total, torch.float32, src_off)
        src.copy_(base)
        bits = src.view(torch.int32)
        for j, p in enumerate(places):
            b = SPECIAL_BITS[(j + rot) % len(SPECIAL_BITS)]
            bits[p] = b - (1 << 32) if b >= 1 << 31 else b
        dst_buf, dst, fill = _guarded(total, torch.float32, dst_off)
        assert src.data_ptr() % 16 == 4 * src_off and dst.data_ptr() % 16 == 4 * dst_off
        TC.collect_record(src.view(n, 965), dst.view(n, 965), _hp())                   # the begin form: every record pointer NULL
        torch.cuda.synchronize()
        want = torch.nan_to_num(src.cpu(), nan=0.0, posinf=float(np.finfo(np.float32).max), neginf=0.0)
        assert _biteq(dst.cpu(), want), (rot, places)
        assert torch.isfinite(dst).all() and _guards_intact(dst_buf, dst, fill)


@pytest.mark.parametrize("n,B", [(1, 1), (1, 257), (255, 1), (256, 255), (257, 256)])
def test_record_transition_ring_pos_and_indices(n, B):
    from isaac_rover_orbit_amd import td3_collect as TC
    g = torch.Generator(device="cuda").manual_seed(n)
    raw = synthetic_rows(n, seed=3)
    rew = torch.randn(n, device="cuda", generator=g)
    for j, b in enumerate((0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000, 0xFFC00001)):
        if j < n:
            rew.view(torch.int32)[(j * 61) % n] = b - (1 << 32) if b >= 1 << 31 else b
    term8 = torch.tensor([0, 1, 2, 255], dtype=torch.uint8, device="cuda").repeat(n // 4 + 1)[:n].contiguous()
    for term in (term8, term8 != 0):
        for mem_rows in (1, 3, 2 ** 25 + 1):
            slot_buf, slot, f_slot = _guarded(n * 965, torch.float32)
            rew_buf, rew_out, f_rew = _guarded(n, torch.float32, 1)
            term_buf, term_out, f_term = _guarded(n, torch.uint8)
            pos_buf, pos, f_pos = _guarded(1, torch.int32)
            idx_buf, idx, f_idx = _guarded(B, torch.int64)
            hp = _hp(seed_lo=42, seed_hi=3)
            counter = (1 << 32) | 7
            TC.collect_record(raw, slot.view(n, 965), hp, counter, rew=rew, terminated=term, rew_out=rew_out, term_out=term_out,
                              ring_pos_entry=pos, ring_pos_value=5, idx_out=idx, mem_rows=mem_rows)
            torch.cuda.synchronize()
            assert _biteq(slot.view(n, 965), torch.nan_to_num(raw, nan=0.0, neginf=0.0))
            assert _biteq(rew_out, rew) and torch.equal(term_out, (term8 != 0).to(torch.uint8))
            assert int(pos) == 5
            want = TC.sample_indices((3 << 32) | 42, counter, B, mem_rows)
            assert idx.cpu().numpy().tolist() == want.tolist() and int(idx.min()) >= 0 and int(idx.max()) < mem_rows
            for buf, view, fill in ((slot_buf, slot, f_slot), (rew_buf, rew_out, f_rew), (term_buf, term_out, f_term),
                                    (pos_buf, pos, f_pos), (idx_buf, idx, f_idx)):
                assert _guards_intact(buf, view, fill)
    # no indices asked for: the index arguments are not read; no transition: only the rows and ring_pos
    slot_buf, slot, f_slot = _guarded(n * 965, torch.float32)
    pos_buf, pos, f_pos = _guarded(1, torch.int32)
    TC.collect_record(raw, slot.view(n, 965), _hp(), 0, ring_pos_entry=pos, ring_pos_value=9)
    torch.cuda.synchronize()
    assert int(pos) == 9 and _biteq(slot.view(n, 965), torch.nan_to_num(raw, nan=0.0, neginf=0.0))
    assert _guards_intact(slot_buf, slot, f_slot) and _guards_intact(pos_buf, pos, f_pos)


# ------------------------------------------------------------------------------------------------------------- the collector
def _step_inputs(n, t):
    raw = synthetic_rows(n, seed=10 + t)
    raw[t % n, 7 + t] = float("nan")
    raw[(t + 3) % n, 964] = float("inf")
    g = torch.Generator(device="cuda").manual_seed(50 + t)
    return raw, torch.randn(n, device="cuda", generator=g), torch.rand(n, device="cuda", generator=g) < 0.3


def test_collector_against_the_spec_and_into_the_update():
    from isaac_rover_orbit_amd import td3_collect as TC
    from isaac_rover_orbit_amd.td3 import FusedTD3, ReplayMemory, explore
    from td3_helpers import nets
    n, M, steps, B = 17, 2, 5, 64
    fused = FusedTD3(*(m.state_dict() for m in nets(seed=3)))
    mem, ref = ReplayMemory(M, n, device="cuda"), ReplayMemory(M, n, device="cpu")
    kw = dict(seed=(7 << 32) | 5, env_id_offset=100, noise_std=0.4, clip=(-0.05, 0.05))
    col = TC.TD3Collector(fused.actor, mem, **kw)
    spec = TC.TorchTD3Collector(lambda o: fused.actor(o.cuda().contiguous()).cpu(), ref, **kw)
    raw0 = _step_inputs(n, 99)[0]
    col.begin(raw0)
    spec.begin({"policy": raw0.cpu()})
    mean, eps = torch.empty(n, 2, device="cuda"), torch.empty(n, 2, device="cuda")
    for t in range(steps):
        scale = (1.0, 0.8, 0.6, None, 0.2)[t]                                           # None: one step past the schedule's end
        k = mem.memory_index
        a = col.act(scale, mean_out=mean, eps_out=eps)
        b = spec.act(scale)
        torch.cuda.synchronize()
        assert _biteq(mean, fused.actor(mem.obs[mem.cursor])) and _biteq(a, mem.actions[k])
        if scale is None:
            assert _biteq(a, mean) and _biteq(a.cpu(), b)
        else:
            assert _biteq(a, explore(mean, 0.4 * eps, scale, -0.05, 0.05))
            assert (a.abs() == 0.05).any()
            # the spec's eps is float64's, rounded: |d eps| <= EPS_TOL goes through x 0.4 x scale.  Where the two results are not
            # clamped to the same bound, one of them lies within reach of (-0.05, 0.05); with |mean| < 0.2 and scale >= 0.2 that
            # means |0.4 eps| < 2, |0.4 eps scale| < 0.5 and a sum below 0.25, so the three roundings move either side by at most
            # 2**-24 x scale, 2**-26 and 2**-27, and the spec's eps is rounded to fp32 once more (2**-24 x 0.4 x scale): under
            # 2**-22 for both sides together
            assert float(mean.abs().max()) < 0.2 and scale >= 0.2
            assert (a.cpu() - b).abs().max() <= 0.4 * scale * EPS_TOL + 2.0 ** -22
        raw, rew, term = _step_inputs(n, t)
        i = col.record(raw, rew, term, B)
        j = spec.record(raw.cpu(), rew.cpu(), term.cpu(), B)
        assert i.dtype == torch.int64 and torch.equal(i.cpu(), j) and int(i.max()) < len(mem) and int(i.min()) >= 0
        for name in ("obs", "rewards", "terminated", "ring_pos"):
            x, y = getattr(mem, name).cpu(), getattr(ref, name)
            assert torch.equal(x, y) and (x.dtype == torch.bool or name == "ring_pos" or _biteq(x, y)), (t, name)
        assert len(mem) == len(ref) == min(t + 1, M) * n
        assert (mem.memory_index, mem.filled, mem.cursor) == (ref.memory_index, ref.filled, ref.cursor)
        assert col.state_dict() == spec.state_dict() == {"seed": (7 << 32) | 5, "counter": 2 * (t + 1), "env_id_offset": 100}
    assert mem.filled and mem._last_next is None and torch.isfinite(mem.obs).all()
    fused.critic_step(mem, i)
    st = fused.stats()
    assert st["bad_index"] == 0 and np.isfinite(st["critic_loss"])
    s, a, r, s2, t_ = mem.gather(i)
    assert torch.isfinite(s).all() and torch.isfinite(s2).all()
    # arguments are validated as RolloutCollector validates them
    raw, rew, term = _step_inputs(n, 0)
    for bad in ((raw[:5], rew, term), (raw.cpu(), rew, term), (raw, rew.double(), term), (raw, rew, term.float()), (raw, rew[:3], term)):
        with pytest.raises(ValueError):
            col.record(*bad)
    with pytest.raises(ValueError):
        col.begin(raw.double())
    with pytest.raises(ValueError):
        TC.TD3Collector(_actor(3), mem)
    with pytest.raises(ValueError):                 # the trainer's optional outputs hold exactly what the kernels write
        fused.critic_step(mem, i, y_out=torch.empty(B - 1, device="cuda"))
    with pytest.raises(ValueError):
        fused.actor_step(mem, i, dact_out=torch.empty(B, device="cuda"))


def test_side_stream_matches_the_default_stream(actor, clean):
    from isaac_rover_orbit_amd import td3_collect as TC
    kw = dict(counter=6, explore=1, noise_std=0.3, noise_scale=0.5)
    want = _act(actor, clean, **kw)
    raw = synthetic_rows(33, seed=4)
    slot, idx = torch.zeros(33, 965, device="cuda"), torch.zeros(65, dtype=torch.int64, device="cuda")
    TC.collect_record(raw, slot, _hp(), 6, idx_out=idx, mem_rows=1000)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _act(actor, clean, **kw)
        slot2, idx2 = torch.zeros(33, 965, device="cuda"), torch.zeros(65, dtype=torch.int64, device="cuda")
        TC.collect_record(raw, slot2, _hp(), 6, idx_out=idx2, mem_rows=1000)
    side.synchronize()
    for k in want:
        assert _biteq(got[k], want[k]), k
    assert _biteq(slot2, slot) and torch.equal(idx2, idx) and _biteq(slot, torch.nan_to_num(raw, nan=0.0, neginf=0.0))
