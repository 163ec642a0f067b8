"""The fused TD3 transition collector (td3_collect, csrc/td3_collect_kernels.hip) at the branches tests/test_gpu_td3_collect.py does
not reach.  At most 97 rows per case (112 for the replicas); every output sits between sentinel guards that are checked after every
launch.  Comparisons are on the bits unless a bound is named.

  * action widths 1, 3, 5, 15 (a half-used Box-Muller pair, epilogue lanes c >= A) at n in {1, 17, 33}: mean against
    rover_policy_forward (bits) and float64 torch (2e-5, the bound of tests/test_gpu_policy.py at this weight scale), eps against
    the float64 spec (EPS_TOL), act against td3.explore
  * the staged rows 0, 4, 8 and 12 bytes off a 16-byte boundary at n = 16 and 17
  * 1, 3 and 5 weight replicas over seven workgroups with NaN behind the last replica
  * degenerate, infinite and overflowing exploration hyper-parameters; a NaN / +inf actor output (NaN stays NaN, as torch.clamp)
  * ids up to 2**31 - 2, seed 2**64 - 1, counters 2**32 - 1, 2**32 and 2**64 - 1, and the split at that offset
  * the record kernel's vector tail of 1, 2 and 3 floats and all sixteen source / destination alignments
  * indices at mem_rows 2**31, 2**32 - 1 and 2**32 with batches 3, 5, 1023, 1025, the grid sized by the batch and by the rows
  * every refusal the header promises: the code, and no output touched
  * TD3Collector: two shards against the whole, the checkpoint, and parameters that move under it
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import random_policy_weights, torch_policy_reference
from rollout_helpers import _biteq, synthetic_rows
from td3_helpers import (EXPLORE_CASES, INDEX_BATCHES, INDEX_MEM_ROWS, TOP_COUNTERS, TOP_OFFSET, TOP_SEED, check_explore_case, nets,
                         same_bits_nan_aware)
from test_gpu_td3_collect import EPS_TOL, SENTINEL, SPECIAL_BITS, _actor, _guarded, _guards_intact, _hp

pytestmark = pytest.mark.gpu

MEAN_TOL = 2e-5        # tests/test_gpu_policy.py: this network, random_policy_weights(scale=3.0), against torch
WEIGHT_SEED, WEIGHT_SCALE = 21, 3.0     # _actor's


@pytest.fixture(scope="module")
def clean():
    """(112, 965) sanitised rows, as a ring slot holds them."""
    return torch.nan_to_num(synthetic_rows(112, seed=0), nan=0.0, neginf=0.0).contiguous()


@pytest.fixture(scope="module")
def actors(clean):
    """A -> (actor of width A, its float64 mean on clean[:33]), computed once."""
    cache = {}

    def get(A):
        if A not in cache:
            ws, bs = random_policy_weights(seed=WEIGHT_SEED, out_dim=A, scale=WEIGHT_SCALE)
            ref = torch_policy_reference([w.astype(np.float64) for w in ws], [b.astype(np.float64) for b in bs],
                                         clean[:33].cpu().numpy().astype(np.float64), final_tanh=False)
            cache[A] = (_actor(A, seed=WEIGHT_SEED), ref)
        return cache[A]
    return get


def _act(actor, rows, counter=0, **hp):
    """One act launch into four guarded (n, A) outputs; the guards are checked here."""
    from isaac_rover_orbit_amd import td3_collect as TC
    n, A = rows.shape[0], actor.out_dim
    bufs = {k: _guarded(n * A, torch.float32) for k in ("mean", "act", "env_act", "eps")}
    o = {k: v[1].view(n, A) for k, v in bufs.items()}
    TC.collect_act(actor, rows, counter, _hp(**hp), o["act"], o["env_act"], mean_out=o["mean"], eps_out=o["eps"])
    torch.cuda.synchronize()
    for k, (buf, view, fill) in bufs.items():
        assert _guards_intact(buf, view, fill), f"{k}: a guard around the (n, A) = ({n}, {A}) output changed"
    return o


# --------------------------------------------------------------------------------------------------------- 1. action widths
@pytest.mark.parametrize("A,n", [(A, n) for A in (1, 3, 5, 15) for n in (1, 17, 33)] + [(2, 33)])
def test_action_widths(actors, clean, A, n):
    from isaac_rover_orbit_amd import rollout as R
    from isaac_rover_orbit_amd import td3_collect as TC
    from isaac_rover_orbit_amd.td3 import explore
    net, ref64 = actors(A)
    rows = clean[:n].contiguous()
    std, scale, low, high = 0.3, 0.7, -0.25, 0.5
    o = _act(net, rows, counter=5, explore=1, noise_std=std, noise_scale=scale, action_low=low, action_high=high, seed_lo=9, seed_hi=5,
             env_id_offset=11)
    assert _biteq(o["mean"], net(rows))
    d_mean = float(np.abs(o["mean"].cpu().numpy().astype(np.float64) - ref64[:n]).max())
    spec = R.standard_normals((5 << 32) | 9, 11 + np.arange(n), 5, A, tag=TC.NOISE_TAG)
    d = np.abs(o["eps"].cpu().numpy().astype(np.float64) - spec)
    print(f"A={A} n={n}: max |mean - float64| = {d_mean:.3e} (bound {MEAN_TOL:.0e}); max |eps_kernel - eps_float64| over {n * A} draws = "
          f"{d.max():.3e}, in the last column {d[:, -1].max():.3e} (bound {EPS_TOL:.3e})")
    assert d_mean <= MEAN_TOL
    assert spec.shape == (n, A) and d.max() <= EPS_TOL                                 # every pair, and the lone cosine column of an odd A
    if A % 2:
        pair = R.standard_normals((5 << 32) | 9, 11 + np.arange(n), 5, A + 1, tag=TC.NOISE_TAG)
        assert np.array_equal(pair[:, :A], spec) and np.abs(o["eps"][:, -1].cpu().numpy() - pair[:, A]).max() > 1e-3   # cosine, not sine
    assert _biteq(o["act"], explore(o["mean"], std * o["eps"], scale, low, high)) and _biteq(o["env_act"], o["act"])
    plain = _act(net, rows, counter=5)
    assert _biteq(plain["mean"], o["mean"]) and _biteq(plain["act"], o["mean"]) and _biteq(plain["env_act"], o["mean"])
    assert bool((plain["eps"] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------ 2. staging alignment
@pytest.mark.parametrize("n", [16, 17])
def test_staging_alignment(actors, clean, n):
    net, _ = actors(3)
    kw = dict(counter=2, explore=1, noise_std=0.3, noise_scale=0.7)
    want = _act(net, clean[:n].contiguous(), **kw)
    assert _biteq(want["mean"], net(clean[:n].contiguous()))
    for off in (0, 1, 2, 3):
        buf = torch.zeros(n * 965 + 8, device="cuda")
        rows = buf[off:off + n * 965].view(n, 965)
        rows.copy_(clean[:n])
        assert rows.data_ptr() % 16 == 4 * off and rows.is_contiguous()
        got = _act(net, rows, **kw)
        for k in want:
            assert _biteq(got[k], want[k]), (off, k)


# -------------------------------------------------------------------------------------------------------------- 3. replicas
def test_number_of_weight_replicas(clean):
    """Seven workgroups over k = 1, 3, 5 replicas; one more replica-sized block of NaN follows the last replica."""
    from isaac_rover_orbit_amd.policy import RoverNet
    src = _actor(2)
    pf = src.packed.numel() // src.n_copies
    results = []
    for k in (1, 3, 5):
        buf = torch.full(((k + 1) * pf,), float("nan"), dtype=torch.float32, device="cuda")
        buf[:k * pf] = src.packed[:pf].repeat(k)
        net = RoverNet.from_packed(src.desc, buf[:k * pf], k)
        o = _act(net, clean, counter=2, explore=1, noise_std=0.3, noise_scale=0.7)
        assert o["mean"].shape == (112, 2)
        for key in o:
            assert torch.isfinite(o[key]).all(), (k, key)
        assert torch.isnan(buf[k * pf:]).all()
        results.append(o)
    for o in results[1:]:
        for key in o:
            assert _biteq(o[key], results[0][key]), key
    assert _biteq(results[0]["mean"], src(clean))


# ------------------------------------------------------------------------------------------------------ 4. hyper-parameters
@pytest.mark.parametrize("name", sorted(EXPLORE_CASES))
def test_exploration_hyper_parameters(actors, clean, name):
    net, _ = actors(2)
    std, scale, low, high = EXPLORE_CASES[name]
    o = _act(net, clean[:33].contiguous(), counter=7, explore=1, noise_std=std, noise_scale=scale, action_low=low, action_high=high)
    assert _biteq(o["mean"], net(clean[:33].contiguous())) and _biteq(o["env_act"], o["act"])
    check_explore_case(name, o["act"], o["mean"], o["eps"])


def test_bounds_are_not_read_without_exploration(actors, clean):
    net, _ = actors(2)
    o = _act(net, clean[:33].contiguous(), explore=0, action_low=1.0, action_high=-1.0, noise_std=0.5)
    assert _biteq(o["act"], o["mean"]) and _biteq(o["env_act"], o["mean"]) and bool((o["eps"] == SENTINEL).all())
    assert _biteq(o["mean"], net(clean[:33].contiguous()))


# ----------------------------------------------------------------------------------------------- 5. non-finite actor output
def test_a_non_finite_actor_output(actors, clean):
    """The last layer's bias is NaN in column 0 and +inf in column 1.  Without exploration both pass through; with it the result is
    td3.explore's: torch.clamp keeps the NaN and brings +inf to the upper bound.  (fminf(fmaxf(NaN, low), high) alone gives `low`:
    before the kernel tested for NaN this test failed with every action of column 0 at -0.5.)"""
    from isaac_rover_orbit_amd.policy import RoverNet
    from isaac_rover_orbit_amd.td3 import explore
    ws, bs = random_policy_weights(seed=WEIGHT_SEED, out_dim=3, scale=WEIGHT_SCALE)
    bs[5][0], bs[5][1] = np.float32("nan"), np.float32("inf")
    bad = RoverNet(ws, bs, n_enc=2, final_act="none")
    good, _ = actors(3)
    rows = clean[:33].contiguous()
    want_mean = good(rows)
    o = _act(bad, rows)
    for k in ("mean", "act", "env_act"):
        assert bool(torch.isnan(o[k][:, 0]).all()) and bool((o[k][:, 1] == float("inf")).all()) and _biteq(o[k][:, 2], want_mean[:, 2]), k
    std, scale, low, high = 0.3, 0.7, -0.5, 0.75
    o = _act(bad, rows, counter=3, explore=1, noise_std=std, noise_scale=scale, action_low=low, action_high=high)
    want = explore(o["mean"], std * o["eps"], scale, low, high)
    assert bool(torch.isnan(want[:, 0]).all()) and bool((want[:, 1] == high).all())     # what the specification says
    print(f"column 0 of act_out: {int(torch.isnan(o['act'][:, 0]).sum())} NaN of 33, {int((o['act'][:, 0] == low).sum())} at action_low")
    assert same_bits_nan_aware(o["act"], want) and same_bits_nan_aware(o["env_act"], want)
    assert bool(torch.isfinite(o["eps"]).all()) and _biteq(o["mean"][:, 2], want_mean[:, 2])


# ---------------------------------------------------------------------------------------------------- 6. top of the ranges
def test_top_of_the_ranges(actors, clean):
    from isaac_rover_orbit_amd import rollout as R
    from isaac_rover_orbit_amd import td3_collect as TC
    net, _ = actors(3)
    rows = clean[:33].contiguous()
    ids = TOP_OFFSET + np.arange(33)
    assert ids[-1] == 2 ** 31 - 2
    kw = dict(explore=1, noise_std=0.3, noise_scale=0.9, seed_lo=0xFFFFFFFF, seed_hi=0xFFFFFFFF)
    worst, seen = 0.0, []
    for counter in TOP_COUNTERS:
        o = _act(net, rows, counter=counter, env_id_offset=TOP_OFFSET, **kw)
        spec = R.standard_normals(TOP_SEED, ids, counter, 3, tag=TC.NOISE_TAG)
        worst = max(worst, float(np.abs(o["eps"].cpu().numpy().astype(np.float64) - spec).max()))
        seen.append(o["eps"])
        lo = _act(net, rows[:16].contiguous(), counter=counter, env_id_offset=TOP_OFFSET, **kw)
        hi = _act(net, rows[16:].contiguous(), counter=counter, env_id_offset=TOP_OFFSET + 16, **kw)
        for k in o:
            assert _biteq(o[k], torch.cat([lo[k], hi[k]])), (counter, k)
    print(f"ids up to 2**31 - 2, seed 2**64 - 1: max |eps_kernel - eps_float64| over {3 * 99} draws = {worst:.3e}; bound {EPS_TOL:.3e}")
    assert worst <= EPS_TOL
    assert not _biteq(seen[0], seen[1]) and not _biteq(seen[1], seen[2])


# ------------------------------------------------------------------------------------------ 7. record tails and alignments
@pytest.mark.parametrize("n", [2, 3, 5])
def test_record_tails_and_alignments(n):
    """n * 965 leaves 2, 3 and 1 floats behind the last 16-byte piece.  The special values sit on those, on the element before them
    and on element 0; every value visits every place over the rotations (on the vector path; the offsets take one rotation each)."""
    from isaac_rover_orbit_amd import td3_collect as TC
    total = n * 965
    tail = total & 3
    assert tail == {2: 2, 3: 3, 5: 1}[n]
    places = [0] + list(range(total - tail - 1, total))
    base = synthetic_rows(n, seed=2).reshape(-1)
    flt_max = float(np.finfo(np.float32).max)
    for src_off in range(4):
        for dst_off in range(4):
            aligned = src_off == 0 and dst_off == 0
            for rot in (range(len(SPECIAL_BITS)) if aligned else (4 * src_off + dst_off,)):
                src_buf, src, _ = _guarded(total, torch.float32, src_off)
                src.copy_(base)
                bits = src.view(torch.int32)
                for j, p in enumerate(places):
                    b = SPECIAL_BITS[(j + rot) % len(SPECIAL_BITS)]
                    bits[p] = b - (1 << 32) if b >= 1 << 31 else b
                dst_buf, dst, fill = _guarded(total, torch.float32, dst_off)
                assert src.data_ptr() % 16 == 4 * src_off and dst.data_ptr() % 16 == 4 * dst_off
                TC.collect_record(src.view(n, 965), dst.view(n, 965), _hp())
                torch.cuda.synchronize()
                want = torch.nan_to_num(src.cpu(), nan=0.0, posinf=flt_max, neginf=0.0)
                assert _biteq(dst.cpu(), want), (src_off, dst_off, rot)
                assert _guards_intact(dst_buf, dst, fill), (src_off, dst_off, rot)


# -------------------------------------------------------------------------------------------------------------- 8. indices
@pytest.mark.parametrize("n,batches", [(1, INDEX_BATCHES), (97, (3,))])
def test_indices_at_the_top_of_mem_rows(n, batches):
    """n = 1 with 1025 indices: the grid is sized by the batch; n = 97 with 3: by the rows."""
    from isaac_rover_orbit_amd import td3_collect as TC
    raw = synthetic_rows(n, seed=3)
    counter = 2 ** 32 - 1
    for mem_rows in INDEX_MEM_ROWS:
        for B in batches:
            slot_buf, slot, f_slot = _guarded(n * 965, torch.float32)
            idx_buf, idx, f_idx = _guarded(B, torch.int64)
            TC.collect_record(raw, slot.view(n, 965), _hp(seed_lo=0xFFFFFFFF, seed_hi=0xFFFFFFFF), counter, idx_out=idx, mem_rows=mem_rows)
            torch.cuda.synchronize()
            want = TC.sample_indices(TOP_SEED, counter, B, mem_rows)
            got = idx.cpu().numpy()
            assert got.tolist() == want.tolist(), (mem_rows, B)
            assert got.min() >= 0 and got.max() < mem_rows
            assert _guards_intact(idx_buf, idx, f_idx) and _guards_intact(slot_buf, slot, f_slot)
            assert _biteq(slot.view(n, 965), torch.nan_to_num(raw, nan=0.0, neginf=0.0))


# ------------------------------------------------------------------------------------------- 9. refusals without a launch
def test_refusals_leave_every_output_alone(clean):
    """ROVER_ERR_INVALID (1) / ROVER_ERR_UNSUPPORTED (4) as include/rover_td3_collect.h names them, on real device buffers: after
    all of them every output still holds its sentinel."""
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    net = _actor(2)
    n = 16
    rows = clean[:n].contiguous()
    outs = {k: torch.full((n * 2 + 8,), SENTINEL, device="cuda") for k in ("mean", "act", "env_act", "eps")}
    hp = _hp(explore=1, noise_std=0.3)
    tanh, wide = _lib.PolicyDesc(), _lib.PolicyDesc.from_buffer_copy(net.desc)
    assert lib.rover_policy_default_desc(C.byref(tanh), 2, 1) == 0
    wide.layers[5].N = 17
    good = dict(actor=C.byref(net.desc), p=net.packed.data_ptr(), hp=C.byref(hp), n=n)

    def act(**kw):
        a = dict(good, **kw)
        return lib.rover_td3_collect_act(a["actor"], a["p"], net.n_copies, a["hp"], C.c_uint64(0), rows.data_ptr(), a["n"],
                                         outs["mean"].data_ptr(), outs["act"].data_ptr(), outs["env_act"].data_ptr(), outs["eps"].data_ptr(), None)
    assert act(hp=C.byref(_hp(explore=2))) == 1
    assert act(hp=C.byref(_hp(explore=1, action_low=1.0, action_high=-1.0))) == 1 and b"action_low" in lib.rover_last_error()
    assert act(actor=C.byref(tanh)) == 4
    assert act(actor=C.byref(wide)) == 4
    assert act(n=0) == 1
    assert act(p=net.packed.data_ptr() + 4) == 1 and b"aligned" in lib.rover_last_error()

    raw = synthetic_rows(n, seed=5)
    ring = torch.full((2 * n * 965,), SENTINEL, device="cuda")
    rew, term = torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    rew_out, term_out = torch.full((n,), SENTINEL, device="cuda"), torch.full((n,), 99, dtype=torch.uint8, device="cuda")
    pos, idx = torch.full((1,), -7, dtype=torch.int32, device="cuda"), torch.full((8,), -7, dtype=torch.int64, device="cuda")
    rgood = dict(raw=raw.data_ptr(), ring=ring.data_ptr(), rew=rew.data_ptr(), term=term.data_ptr(), rew_out=rew_out.data_ptr(),
                 term_out=term_out.data_ptr(), idx=idx.data_ptr(), batch=8, rows=64)

    def rec(**kw):
        a = dict(rgood, **kw)
        return lib.rover_td3_collect_record(a["raw"], n, a["ring"], a["rew"], a["term"], a["rew_out"], a["term_out"], pos.data_ptr(), 3,
                                            a["idx"], a["batch"], a["rows"], C.byref(hp), C.c_uint64(0), None)
    # the slot starts at the raw block's last row: one row of overlap (both pointers are valid device memory of one tensor)
    both = torch.full(((2 * n - 1) * 965,), SENTINEL, device="cuda")
    assert rec(raw=both.data_ptr(), ring=both.data_ptr() + (n - 1) * 965 * 4) == 1 and b"alias" in lib.rover_last_error()
    for missing in ("rew", "term", "rew_out", "term_out"):
        assert rec(**{missing: None}) == 1, missing
    assert rec(batch=0) == 1
    assert rec(rows=0) == 1 and b"mem_rows" in lib.rover_last_error()
    assert rec(rows=2 ** 32 + 1) == 1 and b"mem_rows" in lib.rover_last_error()
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == SENTINEL).all()), k
    assert bool((ring == SENTINEL).all()) and bool((both == SENTINEL).all()) and bool((rew_out == SENTINEL).all())
    assert bool((term_out == 99).all()) and int(pos) == -7 and bool((idx == -7).all())
    assert rec() == 0 and act() == 0                                                   # and the good call of each is accepted
    torch.cuda.synchronize()
    assert int(pos) == 3 and _biteq(outs["mean"][:n * 2].view(n, 2), net(rows))


# ------------------------------------------------------------------------------------------------------ 10. collector level
def _step_inputs(n, t):
    raw = synthetic_rows(n, seed=10 + t)
    raw[t % n, 7 + t] = float("nan")
    g = torch.Generator(device="cuda").manual_seed(50 + t)
    return raw, torch.randn(n, device="cuda", generator=g), torch.rand(n, device="cuda", generator=g) < 0.3


@pytest.fixture(scope="module")
def fused():
    from isaac_rover_orbit_amd.td3 import FusedTD3
    return FusedTD3(*(m.state_dict() for m in nets(seed=3)), policy_delay=1)


def test_two_shards_are_the_whole(fused):
    from isaac_rover_orbit_amd import td3_collect as TC
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    kw = dict(seed=(7 << 32) | 5, noise_std=0.4, clip=(-0.05, 0.05))
    parts = [(slice(0, 33), 0), (slice(0, 16), 0), (slice(16, 33), 16)]
    cols = [TC.TD3Collector(fused.actor, ReplayMemory(4, sl.stop - sl.start, device="cuda"), env_id_offset=off, **kw) for sl, off in parts]
    raw0 = _step_inputs(33, 99)[0]
    for col, (sl, _) in zip(cols, parts):
        col.begin(raw0[sl].contiguous())
    for t in range(3):
        got = []
        for col in cols:
            mean, eps = torch.empty(col.n, 2, device="cuda"), torch.empty(col.n, 2, device="cuda")
            a = col.act(0.8, mean_out=mean, eps_out=eps)
            got.append((a.clone(), eps, mean))
        for j, name in enumerate(("actions", "eps", "mean")):
            assert _biteq(got[0][j], torch.cat([got[1][j], got[2][j]])), (t, name)
        assert bool((got[0][0].abs() == 0.05).any()) and not _biteq(got[0][0], got[0][2].clamp(-0.05, 0.05))
        raw, rew, term = _step_inputs(33, t)
        for col, (sl, _) in zip(cols, parts):
            col.record(raw[sl].contiguous(), rew[sl].contiguous(), term[sl].contiguous())
    assert _biteq(cols[0].memory.actions[:3], torch.cat([cols[1].memory.actions[:3], cols[2].memory.actions[:3]], 1))


def test_checkpoint_reproduces_actions_and_indices(fused):
    from isaac_rover_orbit_amd import td3_collect as TC
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    n, M, B = 17, 3, 37
    kw = dict(seed=(7 << 32) | 5, env_id_offset=100, noise_std=0.4, clip=(-0.05, 0.05))
    col = TC.TD3Collector(fused.actor, ReplayMemory(M, n, device="cuda"), **kw)
    col.begin(_step_inputs(n, 99)[0])

    def step(c, t):
        a = c.act(0.8).clone()
        return a, c.record(*_step_inputs(n, t), B).clone()
    for t in range(2):
        step(col, t)
    sd = col.state_dict()
    assert sd == {"seed": (7 << 32) | 5, "counter": 4, "env_id_offset": 100}
    mem = ReplayMemory(M, n, device="cuda")
    for name in ("obs", "actions", "rewards", "terminated", "ring_pos"):
        getattr(mem, name).copy_(getattr(col.memory, name))
    mem.cursor, mem.memory_index, mem.filled = col.memory.cursor, col.memory.memory_index, col.memory.filled
    fresh = TC.TD3Collector(fused.actor, mem, noise_std=0.4, clip=(-0.05, 0.05))
    fresh.load_state_dict(sd)
    for t in (2, 3):
        (a, i), (b, j) = step(col, t), step(fresh, t)
        assert _biteq(a, b) and torch.equal(i, j), t
        assert int(i.min()) >= 0 and int(i.max()) < len(col.memory) == len(mem)
    for name in ("obs", "actions", "rewards", "ring_pos"):
        assert torch.equal(getattr(mem, name), getattr(col.memory, name)), name
    assert col.state_dict() == fresh.state_dict()


def test_the_collector_sees_live_parameters(fused):
    from isaac_rover_orbit_amd import td3_collect as TC
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    n = 17
    mem = ReplayMemory(3, n, device="cuda")
    col = TC.TD3Collector(fused.actor, mem, noise_std=0.4, clip=(-0.05, 0.05))
    col.begin(_step_inputs(n, 99)[0])
    first, second = torch.empty(n, 2, device="cuda"), torch.empty(n, 2, device="cuda")
    col.act(0.8, mean_out=first)
    slot = mem.obs[mem.cursor].clone()
    assert _biteq(first, fused.actor(slot))
    idx = col.record(*_step_inputs(n, 0), 64)
    mem.obs[mem.cursor].copy_(slot)                                                    # the same rows under the next act
    assert fused.update(mem, idx)                                                      # policy_delay = 1: the actor steps
    col.act(0.8, mean_out=second)
    torch.cuda.synchronize()
    assert _biteq(second, fused.actor(slot)) and not _biteq(second, first)
    assert fused.stats()["bad_index"] == 0
