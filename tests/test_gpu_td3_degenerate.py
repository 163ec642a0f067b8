"""Fused TD3 (include/rover_td3.h) on inputs that are wrong or degenerate, and Polyak's contract.

  D  bad_index: negative, past the filled memory, past 2^31, and a corrupted ring_pos entry, on the critic step and on the actor
     step: the flag is set, it is sticky, and everything else is bit for bit the run with row 0 / ring position 0 in its place;
  E  all rows terminated, none terminated, one row repeated, a memory of one slot and one env, hidden units whose
     pre-activation is exactly 0, NULL against given outputs, a non-default stream;
  F  Polyak bit for bit against torch fp32 at five taus, polyak = 1, and counts that are no multiple of the block.

Comparisons with the float64 spec follow td3_helpers.check; bit comparisons are fused against fused where the test is about
the bits (D, the last two of E) and fused against torch where torch defines them (F)."""
import ctypes as C

import numpy as np
import pytest
import torch

from td3_helpers import assert_same_trainer, check, nets, trainers
from test_gpu_td3_hparams_edges import full_step, gen, shifted
from test_gpu_td3_update import DEV, grads, sample, setup

pytestmark = pytest.mark.gpu

BAD_INDEX_WORD = 3                      # rover_td3_state.bad_index


# ---------------------------------------------------------------------------------------------------------------- D
def one_step(fused, mem, idx, step):
    n = idx.numel()
    if step == "critic":
        out = torch.empty(n, device=DEV)
        fused.critic_step(mem, idx, y_out=out)
    else:
        out = torch.empty(n, 2, device=DEV)
        fused.actor_step(mem, idx, dact_out=out)
    return out


@pytest.mark.parametrize("step", ["critic", "actor"])
@pytest.mark.parametrize("bad", ["minus_one", "len", "two_to_40", "ring_pos_minus_one", "ring_pos_slots"])
def test_bad_index_is_flagged_sticky_and_reads_row_0(bad, step):
    M, N, n, slot = 4, 64, 300, 2
    mem, fused, _ = setup(seed=40, M=M, N=N, steps=6)
    _, clean, _ = setup(seed=40, M=M, N=N, steps=6)
    ok = mem.sample_indices(n, gen(41))
    assert bool((ok // N == slot).any())
    idx, pos = ok.clone(), mem.ring_pos.clone()
    if bad.startswith("ring_pos"):
        mem.ring_pos[slot] = -1 if bad == "ring_pos_minus_one" else mem.slots
        out = one_step(fused, mem, idx, step)
        mem.ring_pos[slot] = 0                                     # the documented substitution: ring position 0
    else:
        where = torch.tensor([0, 137, n - 1], device=DEV)
        idx[where] = {"minus_one": -1, "len": len(mem), "two_to_40": 2 ** 40}[bad]
        out = one_step(fused, mem, idx, step)
        ok[where] = 0                                              # the documented substitution: row 0
    want = one_step(clean, mem, ok, step)
    assert fused.stats()["bad_index"] == 1 and clean.stats()["bad_index"] == 0
    assert bool(torch.isfinite(want).all()) and torch.equal(out, want)
    assert_same_trainer(fused, clean, skip_state_words=(BAD_INDEX_WORD,))
    # sticky: a later clean step leaves the flag up; after the caller zeroes the state a clean step leaves it down
    mem.ring_pos.copy_(pos)
    good = mem.sample_indices(n, gen(42))
    one_step(fused, mem, good, step)
    assert fused.stats()["bad_index"] == 1
    one_step(fused, mem, good, "actor" if step == "critic" else "critic")
    assert fused.stats()["bad_index"] == 1
    fused.state.zero_()
    one_step(fused, mem, good, step)
    st = fused.stats()
    assert st["bad_index"] == 0 and st[f"{step}_step"] == 1


# ---------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("terminated", [True, False])
def test_all_rows_or_no_rows_terminated(terminated):
    mem, fused, specs = setup(seed=46)
    mem.terminated.fill_(terminated)
    idx = shifted(mem).sample_indices(512, gen(44))
    got, r64, _ = full_step(mem, fused, specs, idx)
    r = mem.gather(idx)[2].reshape(-1)
    if terminated:
        assert torch.equal(got["y"], r)                            # y = r + (gamma * 0) * min(...), bit for bit
    else:
        assert not bool((got["y"] == r).any()) and not bool((r64["y"] == r.double()).any())


def test_one_row_repeated_gives_that_rows_gradients():
    """The mean over 1000 copies of a row is the row: float64 runs the row once, torch fp32 the 1000 copies the kernels get."""
    mem, fused, specs = setup(seed=62)
    one = shifted(mem).sample_indices(1, gen(46))
    idx = one.repeat(1000)
    y = torch.empty(1000, device=DEV)
    fused.critic_step(mem, idx, y_out=y)
    gc = fused.unvector(fused.grad)
    fused.actor_step(mem, idx)
    got = {"y": y, "critic_1": gc["critic_1"], "critic_2": gc["critic_2"], "policy": fused.unvector(fused.grad)["policy"]}
    ref = {}
    for dt, rows in ((torch.float64, one), (torch.float32, idx)):
        sp = specs[dt]
        smp = sample(mem, rows, dt)
        st = sp.critic_step(*smp)
        g1, g2 = grads(sp.critic_1), grads(sp.critic_2)
        st.update(sp.actor_step(smp[0]))
        ref[dt] = {"y": st["y"].reshape(-1).expand(1000), "critic_1": g1, "critic_2": g2, "policy": grads(sp.policy), "stats": st}
    r64, r32 = ref[torch.float64], ref[torch.float32]
    for k in ("y", "critic_1", "critic_2", "policy"):
        check(got[k], r64[k], r32[k], what=f"{k} ")
    st = fused.stats()
    for k in ("y_mean", "q1_mean", "q2_mean", "critic_loss", "policy_loss"):
        print(f"{k}: fused {st[k]!r} float64 {r64['stats'][k]!r} torch fp32 {r32['stats'][k]!r}")
        assert st[k] == pytest.approx(r64["stats"][k], rel=1e-3, abs=1e-6), k


@pytest.mark.parametrize("n", [1, 70])
def test_memory_of_one_slot_and_one_env(n):
    mem, fused, specs = setup(seed=63, M=1, N=1, steps=3)         # two ring slots; three adds wrap the ring and the memory
    assert mem.slots == 2 and len(mem) == 1 and mem.filled
    # the one stored reward decides y: shifted by 3 so that y is not, by accident of the draw, next to q (a critic_loss of
    # 1e-4 as the difference of two values near 0.09 is below what the statistics' bound can resolve)
    idx = shifted(mem, 3.0).sample_indices(n, gen(48))
    assert idx.tolist() == [0] * n
    full_step(mem, fused, specs, idx)


def test_units_at_exactly_zero_take_the_negative_slope():
    """A hidden unit with a zero weight row and a zero bias has pre-activation 0 on every row.  torch's LeakyReLU' there is the
    slope (x > 0 ? 1 : 0.01), so that unit's bias gradient is 0.01 x its upstream gradient, not the upstream gradient."""
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    from td3_helpers import fill
    U, E = 37, 11                                                 # a unit of mlp[2] (160) and one of the first encoder layer (80)
    mods = nets(66, DEV)
    with torch.no_grad():
        for m in (mods[0], mods[1]):
            for layer, row in ((m.mlp[2], U), (m.dense_encoder.encoder_layers[0], E)):
                layer.weight[row].zero_()
                layer.bias[row].zero_()
    mem = ReplayMemory(4, 64, device=DEV)
    fill(mem, 6, seed=50)
    fused, specs = trainers(mods)
    got, r64, r32 = full_step(shifted(mem), fused, specs, mem.sample_indices(512, gen(51)))
    for net in ("critic_1", "policy"):
        for name, row in (("mlp.2.bias", U), ("dense_encoder.encoder_layers.0.bias", E)):
            f, w64, w32 = (x[net][name][row:row + 1] for x in (got, r64, r32))
            print(f"{net} {name}[{row}]: fused {float(f)!r} float64 {float(w64)!r} torch fp32 {float(w32)!r}")
            assert float(w64) != 0.0
            check(f, w64, w32, what=f"{net} {name}[{row}] ")
            # the weight row of a unit that is 0 everywhere still gets its gradient; the next layer's column from it gets none
            wname = name.replace("bias", "weight")
            check(got[net][wname][row], r64[net][wname][row], r32[net][wname][row], what=f"{net} {wname}[{row}] ")
            after = "mlp.4.weight" if name.startswith("mlp") else "dense_encoder.encoder_layers.2.weight"
            assert bool((got[net][after][:, row] == 0).all()) and bool((r64[net][after][:, row] == 0).all())


def both(seed=52, n=300):
    mem, a, _ = setup(seed=seed)
    _, b, _ = setup(seed=seed)
    idx = mem.sample_indices(n, gen(seed + 1))
    return mem, a, b, idx, torch.randn(n, 2, device=DEV, generator=gen(seed + 2))


def test_null_outputs_change_nothing():
    mem, a, b, idx, noise = both()
    n = idx.numel()
    y, dact = torch.full((n,), float("nan"), device=DEV), torch.full((n, 2), float("nan"), device=DEV)
    a.critic_step(mem, idx, noise, y_out=y)
    a.actor_step(mem, idx, dact_out=dact)
    b.critic_step(mem, idx, noise)
    b.actor_step(mem, idx)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dact).all())
    assert_same_trainer(a, b)


def test_update_on_a_side_stream_is_bit_identical():
    mem, a, b, idx, noise = both(seed=55)
    a.critic_step(mem, idx, noise)
    a.actor_step(mem, idx)
    a.polyak()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side and side != torch.cuda.default_stream()
        b.critic_step(mem, idx, noise)
        b.actor_step(mem, idx)
        b.polyak()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert_same_trainer(a, b)
    assert a.stats()["actor_step"] == 1 and bool(torch.isfinite(a.params).all())


# ---------------------------------------------------------------------------------------------------------------- F
TAUS = (0.005, 0.05, 0.25, 0.9, 0.995)
# where skrl's float32(1 - tau) is not the kernel's float32(1 - float32(tau)): a recorded fact of float32, see rover_td3.h
SKRL_DIFFERS_AT = (0.9, 0.995)


def moved_trainer(seed, **hp):
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    from td3_helpers import fill
    mem = ReplayMemory(4, 64, device=DEV)
    fill(mem, 6, seed=seed + 1)
    fused, _ = trainers(nets(seed, DEV), **hp)
    idx = mem.sample_indices(256, gen(seed + 2))
    fused.critic_step(mem, idx)
    fused.actor_step(mem, idx)
    assert not torch.equal(fused.target, fused.params)
    return fused


@pytest.mark.parametrize("tau", TAUS)
def test_polyak_is_torch_fp32_for_the_float32_tau(tau):
    fused = moved_trainer(60, polyak=tau)
    tgt, p = fused.target.clone(), fused.params.clone()
    fused.polyak()
    tau32 = float(np.float32(tau))                                 # the number the struct holds, as a Python float
    want = tgt.clone()
    want.mul_(1 - tau32)
    want.add_(tau32 * p)
    assert torch.equal(fused.target, want)
    assert not torch.equal(fused.target, tgt)
    skrl = tgt.clone()                                             # skrl's own form, from the double it was configured with
    skrl.mul_(1 - tau)
    skrl.add_(tau * p)
    same_keep = np.float32(1 - tau) == np.float32(1 - tau32)
    assert torch.equal(fused.target, skrl) == bool(same_keep)
    assert bool(same_keep) == (tau not in SKRL_DIFFERS_AT)
    if not same_keep:
        # float32(tau) is within half an ulp of tau (2^-25 for tau in [0.5, 1)), 1 - tau rounds once more, and each of the
        # two products and the sum rounds once: the two forms stay that close
        tmax, pmax = float(tgt.abs().max()), float(p.abs().max())
        bound = tmax * (2.0 ** -25 + float(np.spacing(np.float32(1 - tau)))) + 2 * float(np.spacing(np.float32(tmax + pmax)))
        assert 0 < float((fused.target - skrl).abs().max()) <= bound


def test_polyak_of_one_copies_the_parameters():
    fused = moved_trainer(61, polyak=1.0)
    fused.polyak()
    assert torch.equal(fused.target, fused.params)


@pytest.mark.parametrize("count", [1, 255, 257])
@pytest.mark.parametrize("offset", [0, 1])
def test_polyak_on_a_short_vector_stops_at_count(count, offset):
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd.td3 import default_hparams
    hp = default_hparams()
    hp.polyak = 0.9
    tau = float(hp.polyak)
    g = gen(62 + count)
    t = torch.randn(offset + count + 64, device=DEV, generator=g)
    p = torch.randn(offset + count + 64, device=DEV, generator=g)
    orig, want = t.clone(), t.clone()
    want[offset:offset + count].mul_(1 - tau)
    want[offset:offset + count].add_(tau * p[offset:offset + count])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().rover_td3_polyak(C.byref(hp), t[offset:].data_ptr(), p[offset:].data_ptr(), count, stream), "rover_td3_polyak")
    assert torch.equal(t, want)                                   # the floats before `offset` and from `count` on are untouched
    assert not bool((t[offset:offset + count] == orig[offset:offset + count]).any())
