"""TD3 / SAC behind skrl's running state scaler on the GPU (include/rover_offpolicy_scaled.h, isaac_rover_orbit_amd.offpolicy_scaled):

  * rover_offpolicy_stage_resolve against a numpy restatement: a wrapped ring, repeated indices, an index at valid_rows, a negative
    one and a ring position out of range (row 0, a sticky bad_index), n in {1, 255, 256, 257}
  * rover_offpolicy_stage_rows bit for bit against DeviceScaler.forward on the gathered rows: every source phase against every
    destination phase, NaN / inf / the clip's edges, widths 1, 4, 965, 1024, nothing written outside the n rows
  * the device statistics after two scaled updates against the float64 spec at rtol 1e-12 (tests/test_gpu_ppo_scaled.py's bound for
    this scaler), n in {2, 65, 513}, train_next_states on and off
  * an identity block (mean 0, var 1, clip inf, frozen) leaves every vector of the trainer bit-identical to the unscaled update
  * three scaled updates at n = 513 track the float64 spec within td3_helpers.check (4x torch fp32's own error plus a 1e-5 floor)
  * the collectors with a state_scaler equal the unscaled collector on a slot that holds DeviceScaler.forward(rows); the ring keeps
    the raw rows; state_scaler=None is the collector without the argument
  * a frozen one-row update, the two-row rule, no host synchronisation, the checkpoint entry, the examples with --preprocess running

Every input is made on the CPU and copied to the device, as in tests/test_gpu_sac_update.py."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import sac_helpers
import td3_helpers
from td3_helpers import check, fill, same_bits_nan_aware

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
OBS = 965
SENTINEL = 777.0


def memory(seed, M=4, N=9, steps=6):
    """td3_helpers.fill on the CPU (its draws depend on the generator's device), copied to the GPU.  Six adds into four memory slots:
    the memory and the five-slot ring have wrapped, memory slot 0 holds its s in the last ring slot and its s' in slot 0."""
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    cpu = ReplayMemory(M, N, device="cpu")
    fill(cpu, steps, seed=seed)
    mem = ReplayMemory(M, N, device=DEV)
    for name in ("obs", "actions", "rewards", "terminated", "ring_pos"):
        getattr(mem, name).copy_(getattr(cpu, name))
    mem.memory_index, mem.filled, mem.cursor = cpu.memory_index, cpu.filled, cpu.cursor
    return mem


def indices(mem, n, seed):
    return torch.randint(0, len(mem), (n,), generator=torch.Generator().manual_seed(seed)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == torch.bool else t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def biteq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def params(m):
    return {k: p.detach().clone() for k, p in m.named_parameters()}


# ------------------------------------------------------------------------------------------------------------------- resolve
def resolve_numpy(idx, valid, N, slots, pos, act, rew, term):
    """The header's rules restated: (rows_s, rows_next, actions, rewards, terminated, bad)."""
    i = idx.astype(np.int64).copy()
    bad = (i < 0) | (i >= valid)
    i[bad] = 0
    k, e = i // N, i % N
    p = pos[k].astype(np.int64)
    bad_p = (p < 0) | (p >= slots)
    p[bad_p] = 0
    return p * N + e, ((p + 1) % slots) * N + e, act.reshape(-1, act.shape[-1])[i], rew.reshape(-1)[i], term.reshape(-1)[i], bool((bad | bad_p).any())


def run_resolve(mem, idx, bad):
    from isaac_rover_orbit_amd import offpolicy_scaled as OS
    st = OS.StagedBatch(idx.numel(), DEV)
    st.actions.fill_(SENTINEL); st.rewards.fill_(SENTINEL)
    OS.stage_resolve(mem, idx, st, bad)
    want = resolve_numpy(idx.cpu().numpy(), len(mem), mem.num_envs, mem.slots, mem.ring_pos.cpu().numpy(), mem.actions.cpu().numpy(),
                         mem.rewards.cpu().numpy(), mem.terminated.cpu().numpy())
    assert np.array_equal(st.rows_s.cpu().numpy(), want[0]) and np.array_equal(st.rows_next.cpu().numpy(), want[1])
    assert np.array_equal(st.actions[0].cpu().numpy().view(np.int32), np.ascontiguousarray(want[2]).view(np.int32))
    assert np.array_equal(st.rewards[0].cpu().numpy().view(np.int32), np.ascontiguousarray(want[3]).view(np.int32))
    assert np.array_equal(st.terminated[0].cpu().numpy(), want[4])
    assert len(st) == idx.numel() and int(st.ring_pos[0]) == 0 and torch.equal(st.arange.cpu(), torch.arange(idx.numel()))
    return st, want


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_resolve_against_numpy_with_a_wrapped_ring_and_bad_entries(n):
    mem = memory(1)
    assert mem.ring_pos.tolist() == [4, 0, 2, 3] and mem.slots == 5
    with torch.no_grad():                                  # bit patterns a copy has to keep
        mem.actions[0, 0, 0], mem.actions[1, 2, 1], mem.rewards[0, 1] = -0.0, float("nan"), float("-inf")
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    idx = indices(mem, n, 3 + n)
    idx[0] = 1                                             # memory slot 0: s in the last ring slot, s' in slot 0
    st, want = run_resolve(mem, idx, bad)
    assert want[0][0] == 4 * 9 + 1 and want[1][0] == 1 and int(bad) == 0 and not want[5]
    if n > 1:
        assert len(set(idx.tolist())) < n                  # repeated indices
    # an index at valid_rows, a negative one, a ring position out of range: row 0 / ring slot 0, and the word is set
    spoiled = idx.clone()
    spoiled[0] = len(mem)
    broken = memory(1)
    if n > 1:
        spoiled[7], spoiled[9] = -1, 2 * 9 + 4
        broken.ring_pos[2] = broken.slots
    st, want = run_resolve(broken, spoiled, bad)
    assert want[5] and int(bad) == 1 and want[0][0] == broken.ring_pos[0].item() * 9
    if n > 1:
        assert want[0][7] == want[0][0] and want[0][9] == 4 and want[1][9] == 9 + 4
    run_resolve(mem, idx, bad)                             # a clean call does not clear it
    assert int(bad) == 1


# ---------------------------------------------------------------------------------------------------------------- stage rows
def ring_rows(R, w, seed, scaler):
    """(R, w) rows of scale 2 about 0.5 with NaN, +-inf and values at (row 3), one ulp past (row 4) and just inside (row 6)
    mean +- clip * (sd + eps)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, w, generator=g) * 2.0 + 0.5
    scaler.train(x.to(DEV))
    x[1, 0], x[2, w - 1], x[5, w // 2] = float("nan"), float("inf"), float("-inf")
    mu = scaler.running_mean.float().cpu()
    sd = scaler.running_variance.float().sqrt().cpu() + 1e-8
    for j, c in enumerate(range(0, w, max(1, w // 8))):
        edge = (mu[c] + (5.0 if j % 2 else -5.0) * sd[c]).reshape(1)
        x[3, c] = edge
        x[4, c] = torch.nextafter(edge, edge * 2.0 if j % 2 else edge - 1.0)
        x[6, c] = mu[c] + (4.9999 if j % 2 else -4.9999) * sd[c]       # well inside: not clipped
    return x


@pytest.mark.parametrize("offsets", [(0, 0), (1, 3)])
@pytest.mark.parametrize("n", [1, 5, 64, 65])
@pytest.mark.parametrize("w", [1, 4, 965, 1024])
def test_stage_rows_equals_forward_on_the_gathered_rows(w, n, offsets):
    from isaac_rover_orbit_amd import offpolicy_scaled as OS
    from isaac_rover_orbit_amd.scaler import DeviceScaler
    R = 45                                                 # a ring of 5 slots x 9 envs
    sc = DeviceScaler(w, DEV)
    rows = ring_rows(R, w, 100 + w, sc)
    x_off, o_off = offsets
    xbuf = torch.full((R * w + 8,), SENTINEL, device=DEV)
    x = xbuf[x_off:x_off + R * w].view(R, w)
    x.copy_(rows)
    keep = xbuf.clone()
    # destination row i of phase i % 4 (at w % 4 == 1) takes a source row of phase (i // 4) % 4: all 16 pairs within 16 rows
    src = torch.tensor([((i // 4) % 4 + 4 * ((7 * i) % (R // 4))) % R for i in range(n)], dtype=torch.int64)
    if n >= 16:
        assert len({(int(s) % 4, i % 4) for i, s in enumerate(src)}) == 16
    if n > 1:
        src[n - 1] = src[0]                                # a repeated entry is read twice
    src = src.to(DEV)
    obuf = torch.full(((n + 2) * w + 8,), SENTINEL, device=DEV)
    out = obuf[o_off:o_off + (n + 2) * w].view(n + 2, w)
    OS.stage_rows(sc, x, src, out[:n])
    want = sc.forward(x[src].contiguous())
    assert same_bits_nan_aware(out[:n], want)
    if n >= 64:                                            # the rows with NaN, +-inf and the clip's edges are among the sources
        assert {1, 2, 3, 4, 5, 6} <= set(src.tolist())
        assert bool(torch.isnan(want).any()) and bool((want == 5.0).any()) and bool((want == -5.0).any())
        assert bool(((want.abs() < 5.0) & (want.abs() > 4.999)).any())
    # nothing but the n rows is written, and the ring is not
    assert bool((obuf[:o_off] == SENTINEL).all()) and bool((obuf[o_off + n * w:] == SENTINEL).all())
    assert same_bits_nan_aware(xbuf, keep)


def test_stage_rows_refuses_overlap_and_flags_a_source_row_out_of_range():
    from isaac_rover_orbit_amd import _lib, offpolicy_scaled as OS
    from isaac_rover_orbit_amd.scaler import DeviceScaler
    sc = DeviceScaler(OBS, DEV)
    x = torch.randn(12, OBS, generator=torch.Generator().manual_seed(5)).to(DEV)
    src = torch.tensor([3, -1, 12, 0], dtype=torch.int64, device=DEV)
    out = torch.empty(4, OBS, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    OS.stage_rows(sc, x, src, out, bad)
    assert int(bad) == 1 and biteq(out, sc.forward(x[torch.tensor([3, 0, 0, 0], device=DEV)].contiguous()))
    bad.zero_()
    OS.stage_rows(sc, x, src[:1], out, bad)
    assert int(bad) == 0
    with pytest.raises(_lib.RoverHipError):
        OS.stage_rows(sc, x, src[:1], x[4:8])
    with pytest.raises(ValueError):
        OS.stage_rows(sc, x, src, out[:3])
    with pytest.raises(ValueError):
        OS.stage_rows(sc, x, src.int(), out)


# ------------------------------------------------------------------------------------------------------------- the trainers
def setup(algo, seed, **kw):
    """(memory, fused scaled trainer, {dtype: scaled spec}) with the same networks; the specs run on the device."""
    from isaac_rover_orbit_amd import offpolicy_scaled as OS
    h = td3_helpers if algo == "td3" else sac_helpers
    mods = [m.to(DEV) for m in h.nets(seed, "cpu")]
    fused, specs = h.trainers(mods)
    Fused, Torch = (OS.FusedScaledTD3, OS.TorchScaledTD3) if algo == "td3" else (OS.FusedScaledSAC, OS.TorchScaledSAC)
    return memory(seed + 1), Fused(fused, **kw), {dt: Torch(sp, **kw) for dt, sp in specs.items()}


def extra(algo, n, seed):
    """The update's third argument: TD3's smoothing noise (n, 2) or SAC's draws (n, 4)."""
    if algo == "sac":
        return sac_helpers.draws(n, seed).to(DEV)
    return (torch.randn(n, 2, generator=torch.Generator().manual_seed(seed)) * 0.2).to(DEV)


@pytest.mark.parametrize("train_next", [True, False])
@pytest.mark.parametrize("n", [2, 65, 513])
@pytest.mark.parametrize("algo", ["td3", "sac"])
def test_statistics_after_two_updates_equal_the_float64_spec(algo, n, train_next):
    mem, scaled, specs = setup(algo, 2, train_next_states=train_next)
    s64 = specs[F64]
    for step in range(2):
        idx = indices(mem, n, 10 * n + step)
        scaled.update(mem, idx, extra(algo, n, 5 + step))
        s64.sample(mem, idx)                               # the spec's scaler part: the statistics do not read the networks
    block = scaled.state_scaler.block.cpu().numpy()
    sp = s64.state_preprocessor
    np.testing.assert_allclose(block[:OBS], sp.running_mean.cpu().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(block[OBS:2 * OBS], sp.running_variance.cpu().numpy(), rtol=1e-12)
    assert block[2 * OBS] == float(sp.current_count) == 1 + 2 * n * (2 if train_next else 1)
    st = scaled.stats()
    assert st["critic_step"] == 2 and st["bad_index"] == 0 and bool(torch.isfinite(scaled.params).all())
    # the staged batch holds the rows as the final statistics of each side left them
    rows = mem.obs.reshape(-1, OBS)
    assert biteq(scaled.staged.obs[1], scaled.state_scaler.forward(rows[scaled.staged.rows_next].contiguous()))


@pytest.mark.parametrize("algo,steps", [("td3", 4), ("sac", 2)])
def test_identity_block_leaves_the_update_bit_identical(algo, steps):
    from isaac_rover_orbit_amd import offpolicy_scaled as OS
    from isaac_rover_orbit_amd.scaler import DeviceScaler
    h = td3_helpers if algo == "td3" else sac_helpers
    mods = [m.to(DEV) for m in h.nets(4, "cpu")]
    plain, inner = h.trainers(mods)[0], h.trainers(mods)[0]
    sc = DeviceScaler(OBS, DEV, clip_threshold=float("inf"))           # mean 0, var 1: (x - 0) / (1 + 1e-8) is x in fp32
    scaled = (OS.FusedScaledTD3 if algo == "td3" else OS.FusedScaledSAC)(inner, state_scaler=sc)
    mem = memory(5)
    n = 300
    block = sc.block.clone()
    for step in range(steps):
        idx, e = indices(mem, n, 40 + step), extra(algo, n, 50 + step)
        plain.update(mem, idx, e)
        scaled.update(mem, idx, e, train=False)
    h.assert_same_trainer(plain, inner)
    assert torch.equal(sc.block, block) and plain.stats()["actor_step"] == 2
    assert biteq(scaled.staged.obs[0], mem.obs.reshape(-1, OBS)[scaled.staged.rows_s])


def sac_margin(spec, mem, idx, eps):
    """sac_helpers.update_with_margin for the scaled spec: the update in its pieces on the standardised sample."""
    s, a, r, s2, t = spec.sample(mem, idx)
    tr = spec.inner
    m = sac_helpers.decision_margin(tr, s2, eps[:, 0:2], tr.target_critic_1, tr.target_critic_2)
    tr.critic_step(s, a, r, s2, t, eps[:, 0:2])
    m = min(m, sac_helpers.decision_margin(tr, s, eps[:, 2:4], tr.critic_1, tr.critic_2))
    tr.policy_step(s, eps[:, 2:4])
    tr.polyak()
    return m


# SAC's seed picked with the float64 scaled spec on the CPU among 0 .. 15: the margin below over the three updates is 2.6e-4 there
# (seeds 1, 7 and 9 give 2.3e-4, seed 6 gives 5.8e-6).  TD3 has no such decision in a gradient: min and clamp only shape y.
SAC_SEED = 12
TD3_SEED = 6


def test_three_scaled_td3_updates_track_the_float64_spec():
    mem, scaled, specs = setup("td3", TD3_SEED)
    n = 513
    for step in range(3):
        idx, noise = indices(mem, n, 60 + step), extra("td3", n, 70 + step)
        scaled.update(mem, idx, noise)
        for sp in specs.values():
            sp.update(mem, idx, noise)
    st = scaled.stats()
    assert (st["critic_step"], st["actor_step"], st["bad_index"]) == (3, 1, 0) and scaled.critic_updates == 3
    p, t = scaled.unvector(scaled.params), scaled.unvector(scaled.target)
    s64, s32 = specs[F64].inner, specs[F32].inner
    for k in ("policy", "critic_1", "critic_2"):
        check(p[k], params(getattr(s64, k)), params(getattr(s32, k)), what=f"{k} ")
        check(t[k], params(getattr(s64, "target_" + k)), params(getattr(s32, "target_" + k)), what=f"target_{k} ")


def test_three_scaled_sac_updates_track_the_float64_spec():
    mem, scaled, specs = setup("sac", SAC_SEED)
    n = 513
    margin = math.inf
    for step in range(3):
        idx, eps = indices(mem, n, 80 + step), extra("sac", n, 1000 * SAC_SEED + step)
        scaled.update(mem, idx, eps)
        margin = min(margin, sac_margin(specs[F64], mem, idx, eps))
        specs[F32].update(mem, idx, eps)
    # no clamp and no min decision of any row lies within 1e-4 of flipping (tests/test_gpu_sac_update.py's rule)
    print("margin", margin)
    assert margin >= 1e-4, margin
    st = scaled.stats()
    assert (st["critic_step"], st["actor_step"], st["entropy_step"], st["bad_index"]) == (3, 3, 3, 0)
    p, t = scaled.unvector(scaled.params), scaled.unvector(scaled.target)
    s64, s32 = specs[F64].inner, specs[F32].inner
    for k in ("policy", "critic_1", "critic_2"):
        check(p[k], params(getattr(s64, k)), params(getattr(s32, k)), what=f"{k} ")
    for k in ("critic_1", "critic_2"):
        check(t[k], params(getattr(s64, "target_" + k)), params(getattr(s32, "target_" + k)), what=f"target_{k} ")
    check(p["log_entropy_coefficient"], s64.log_entropy_coefficient.detach().reshape(1), s32.log_entropy_coefficient.detach().reshape(1),
          what="log_alpha")


@pytest.mark.parametrize("algo", ["td3", "sac"])
def test_frozen_one_row_update_two_row_rule_and_no_synchronisation(algo):
    mem, scaled, _ = setup(algo, 7)
    one = indices(mem, 1, 90)
    with pytest.raises(ValueError):                        # before any launch: nothing is staged, nothing stepped
        scaled.update(mem, one, extra(algo, 1, 91))
    assert scaled.staged is None and scaled.stats()["critic_step"] == 0
    block = scaled.state_scaler.block.clone()
    scaled.update(mem, one, extra(algo, 1, 91), train=False)
    st = scaled.stats()
    assert st["critic_step"] == 1 and math.isfinite(st["critic_loss"]) and biteq(scaled.state_scaler.block, block)
    n = 128
    idx, e = indices(mem, n, 92), extra(algo, n, 93)
    scaled.update(mem, idx, e)                             # the workspaces and the staged batch are allocated here
    staged = scaled.staged
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        scaled.update(mem, idx, e)
        scaled.update(mem, idx, e, train=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert scaled.staged is staged and float(scaled.state_scaler.current_count) == 1 + 4 * n
    # the staging's bad_index is OR-ed into the report and stays
    spoiled = idx.clone()
    spoiled[5] = len(mem)
    scaled.update(mem, spoiled, e)
    assert scaled.stats()["bad_index"] == 1 and scaled.fused.stats()["bad_index"] == 0
    scaled.update(mem, idx, e)
    assert scaled.stats()["bad_index"] == 1


@pytest.mark.parametrize("algo", ["td3", "sac"])
def test_checkpoint_round_trip_of_the_fused_scaled_trainer(algo):
    from isaac_rover_orbit_amd import offpolicy_scaled as OS
    mem, scaled, _ = setup(algo, 8)
    n = 64
    scaled.update(mem, indices(mem, n, 94), extra(algo, n, 95))
    ck = scaled.state_dict()
    entry = ck["state_preprocessor"]
    assert tuple(entry) == ("running_mean", "running_variance", "current_count") and list(ck)[-1] == "state_preprocessor"
    assert entry["running_mean"].shape == (OBS,) and entry["running_variance"].shape == (OBS,) and entry["current_count"].shape == ()
    assert float(entry["current_count"]) == 1 + 2 * n
    cls = type(scaled)
    back = cls.from_checkpoint(ck)
    assert biteq(back.state_scaler.block, scaled.state_scaler.block) and biteq(back.params, scaled.params) and biteq(back.target, scaled.target)
    fresh = cls.from_checkpoint({k: v for k, v in ck.items() if k != "state_preprocessor"})
    b = fresh.state_scaler.block.cpu()
    assert not b[:OBS].any() and bool((b[OBS:] == 1).all())
    with pytest.raises(TypeError):
        cls(object())
    assert isinstance(scaled.fused, OS.FusedTD3 if algo == "td3" else OS.FusedSAC) and scaled.actor is scaled.fused.actor


# --------------------------------------------------------------------------------------------------------------- collectors
def raw_rows(n, seed):
    raw = torch.randn(n, OBS, generator=torch.Generator().manual_seed(seed)) * 2.0 + 0.3
    raw[seed % n, 11] = float("-inf")
    raw[(seed + 1) % n, 964] = float("nan")
    return raw.to(DEV)


@pytest.fixture(scope="module")
def trained_scaler():
    from isaac_rover_orbit_amd.scaler import DeviceScaler
    sc = DeviceScaler(OBS, DEV)
    sc.train((torch.randn(64, OBS, generator=torch.Generator().manual_seed(12)) * 3.0 + 0.5).to(DEV))
    return sc


COLLECTORS = ["td3", "td3_gaussian", "explorer_ou", "explorer_random", "sac", "sac_mean", "sac_random"]


def make_collector(kind, fused, mem, **kw):
    """(collector, act(t, mean_out)) of one kind on ``mem``."""
    from isaac_rover_orbit_amd.sac_collect import SACCollector
    from isaac_rover_orbit_amd.td3_collect import TD3Collector
    from isaac_rover_orbit_amd.td3_explore import TD3Explorer
    if kind.startswith("sac"):
        col = SACCollector(fused.actor, fused.log_std, mem, seed=3, random_timesteps=1 if kind == "sac_random" else 0, **kw)
        return col, lambda t, mean: col.act(t, deterministic=kind == "sac_mean", mean_out=mean)
    if kind.startswith("explorer"):
        col = TD3Explorer(fused.actor, mem, seed=3, noise="ou", random_timesteps=1 if kind == "explorer_random" else 0, **kw)
        return col, lambda t, mean: col.act(t, 10, mean_out=mean)
    col = TD3Collector(fused.actor, mem, seed=3, noise_std=0.3 if kind == "td3_gaussian" else 0.0, **kw)
    return col, lambda t, mean: col.act(0.5 if kind == "td3_gaussian" else None, mean_out=mean)


@pytest.fixture(scope="module")
def actors():
    return {"td3": td3_helpers.trainers([m.to(DEV) for m in td3_helpers.nets(9, "cpu")])[0],
            "sac": sac_helpers.trainers([m.to(DEV) for m in sac_helpers.nets(9, "cpu", log_std=(-0.5, -1.5))])[0]}


@pytest.mark.parametrize("kind", COLLECTORS)
def test_collectors_with_a_scaler_equal_the_unscaled_collector_on_standardised_rows(kind, actors, trained_scaler):
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    fused = actors["sac" if kind.startswith("sac") else "td3"]
    n, sc = 7, trained_scaler
    block = sc.block.clone()
    out = {}
    for name, kw in (("scaled", {"state_scaler": sc}), ("plain", {}), ("none", {"state_scaler": None}), ("raw", {})):
        mem = ReplayMemory(3, n, device=DEV)
        col, act = make_collector(kind, fused, mem, **kw)
        col.begin(raw_rows(n, 20))
        steps = []
        for t in range(2):
            slot, k = mem.cursor, mem.memory_index
            stored = mem.obs[slot].clone()
            assert biteq(stored, torch.nan_to_num(raw_rows(n, 20 + t), nan=0.0, posinf=3.4028234663852886e38, neginf=0.0))
            if name == "plain":                            # the unscaled collector on a slot that already holds forward(rows)
                mem.obs[slot].copy_(sc.forward(stored))
            mean = torch.full((n, 2), SENTINEL, device=DEV)
            a = act(t, mean).clone()
            if name == "scaled":
                assert biteq(mem.obs[slot], stored)        # the ring slot keeps the raw rows
            steps.append((a, mem.actions[k].clone(), mean))
            col.record(raw_rows(n, 21 + t), torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.bool, device=DEV))
        out[name] = steps
        assert (col._scaled is None) == (name != "scaled")
    for t in range(2):
        for x, y in zip(out["scaled"][t], out["plain"][t]):
            assert same_bits_nan_aware(x, y), (kind, t)
        for x, y in zip(out["none"][t], out["raw"][t]):    # state_scaler=None: the collector without the argument
            assert same_bits_nan_aware(x, y), (kind, t)
    acted = 1 if kind.endswith("random") else 0            # the random step reads no rows: the same action either way
    assert not same_bits_nan_aware(out["scaled"][acted][0], out["raw"][acted][0])
    if kind.endswith("random"):
        assert biteq(out["scaled"][0][0], out["raw"][0][0])
    assert biteq(sc.block, block)                          # acting never trains


# ----------------------------------------------------------------------------------------------------------------- examples
def load_example(name):
    spec = importlib.util.spec_from_file_location("example_" + name[:2], os.path.join(ROOT, "examples", name))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


@pytest.mark.parametrize("update,rollout", [("fused", "torch"), ("torch", "torch")])
@pytest.mark.parametrize("name", ["07_train_td3.py", "09_train_sac.py"])
def test_example_runs_with_the_running_scaler_on_the_torch_paths(name, update, rollout, tmp_path):
    ex = load_example(name)
    out, save = tmp_path / "log.jsonl", tmp_path / "a.pt"
    ex.main(["--preprocess", "running", "--update", update, "--rollout", rollout, "--num_envs", "8", "--batch_size", "16",
             "--memory_size", "4", "--log_every", "3", "--timesteps", "3", "--out", str(out), "--save", str(save)])
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    assert len(lines) == 1 and lines[0]["timestep"] == 3 and math.isfinite(lines[0]["critic_loss"])
    ck = torch.load(save, map_location="cpu", weights_only=False)
    entry = ck["state_preprocessor"]
    assert tuple(entry) == ("running_mean", "running_variance", "current_count")
    assert float(entry["current_count"]) == 1 + 3 * 2 * 16 and bool(entry["running_mean"].any())
    again = tmp_path / "b.pt"
    ex.main(["--preprocess", "running", "--update", update, "--rollout", rollout, "--num_envs", "8", "--batch_size", "16",
             "--memory_size", "4", "--timesteps", "1", "--learning_starts", "2", "--resume", str(save), "--save", str(again)])
    back = torch.load(again, map_location="cpu", weights_only=False)
    for k, v in entry.items():
        assert torch.equal(back["state_preprocessor"][k], v), k
    for k, v in ck["critic_1"].items():
        assert torch.equal(back["critic_1"][k], v), k


@pytest.mark.parametrize("name", ["07_train_td3.py", "09_train_sac.py"])
def test_example_runs_saves_and_resumes_with_the_running_scaler(name, tmp_path):
    ex = load_example(name)
    out, save, again = tmp_path / "log.jsonl", tmp_path / "a.pt", tmp_path / "b.pt"
    common = ["--preprocess", "running", "--update", "fused", "--rollout", "fused", "--num_envs", "8", "--batch_size", "16",
              "--memory_size", "4", "--log_every", "4"]
    ex.main(common + ["--timesteps", "4", "--out", str(out), "--save", str(save)])
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    assert len(lines) == 1 and lines[0]["timestep"] == 4 and lines[0]["critic_step"] == 4
    assert math.isfinite(lines[0]["critic_loss"]) and lines[0].get("bad_index", 0) == 0
    ck = torch.load(save, map_location="cpu", weights_only=False)
    entry = ck["state_preprocessor"]
    assert float(entry["current_count"]) == 1 + 4 * 2 * 16 and bool(entry["running_mean"].any())
    # stop and resume: the statistics of the checkpoint are the run's (no update before learning_starts: they are written back as read)
    ex.main(common + ["--timesteps", "1", "--learning_starts", "2", "--resume", str(save), "--save", str(again)])
    back = torch.load(again, map_location="cpu", weights_only=False)
    for k, v in entry.items():
        assert torch.equal(back["state_preprocessor"][k], v), k
    for k, v in ck["policy"].items():
        assert torch.equal(back["policy"][k], v), k
