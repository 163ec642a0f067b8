"""Fused SAC (include/rover_sac.h) on inputs that are wrong or degenerate.

  D  log_std on and one float past its clamp's bounds with all draws zero, where dL/dlog_std is -alpha whatever the networks
     are; a NaN draw; all rows terminated, none terminated, one row repeated; bad_index: negative, past the filled memory, past
     2^31, and a corrupted ring_pos entry, on the critic step and on the policy step: the flag is set, it is sticky, and
     everything else is bit for bit the run with row 0 / ring position 0 in its place; NULL against given outputs, a
     non-default stream, the replica count.

Comparisons with the float64 spec follow td3_helpers.check and test_gpu_sac_hparams_edges.full_step; bit comparisons are fused
against fused where the test is about the bits.  Every input is made on the CPU and copied to the device."""
import math

import numpy as np
import pytest
import torch

from sac_helpers import assert_same_trainer, check, grads, nets, sample, specs, trainers
from test_gpu_sac_hparams_edges import HIDDEN, MARGIN, batch, full_step, hp_modules, memory
from test_gpu_sac_update import DEV, F32, F64, policy_case

pytestmark = pytest.mark.gpu

BAD_INDEX_WORD = 3                      # rover_sac_state.bad_index
LN_2PI = math.log(2.0 * math.pi)


# ---------------------------------------------------------------------------------------------------------------- log_std
ON_BOUNDS = (2.0, -20.0)
PAST_BOUNDS = (float(np.nextafter(np.float32(2.0), np.float32(np.inf))), float(np.nextafter(np.float32(-20.0), np.float32(-np.inf))))


@pytest.mark.parametrize("log_std", [ON_BOUNDS, PAST_BOUNDS], ids=["on_bounds", "one_float_past"])
def test_log_std_on_and_just_past_its_bounds_with_zero_draws(log_std):
    """With eps = 0: x = mu, |mu| < 1, t = 0 and per row dL/dls = -alpha / B, so dL/dlog_std[c] = -alpha up to the reduction's
    rounding, whatever the networks are -- unless the parameter is outside [-20, 2], where clamp's backward gives exactly 0.  The
    bounds are inclusive, as torch.clamp's backward has them.  (No comparison of t-dependent values with nonzero draws at
    log_std = -20: there mu + sigma eps rounds to mu in fp32, and fp32 and float64 legitimately disagree by O(1).)"""
    assert PAST_BOUNDS[0] > 2.0 and PAST_BOUNDS[1] < -20.0 and np.float32(PAST_BOUNDS[0]) == PAST_BOUNDS[0]
    mem = memory(81)
    fused, sp = trainers([m.to(DEV) for m in nets(80, "cpu", log_std=log_std)])
    n = 300
    idx = batch(mem, n, 82)[0]
    eps = torch.zeros(n, 4, device=DEV)
    t = fused.tail
    assert fused.params[t:t + 2].tolist() == list(log_std)
    before = [v[t:t + 2].clone() for v in (fused.params, fused.adam_m, fused.adam_v)]
    alpha = float(sp[F64].entropy_coefficient)                                       # the one this step uses
    got, out = policy_case(mem, fused, sp, idx, eps)
    r64, r32 = out[F64], out[F32]
    assert bool((r64["x"].abs() < 1).all()) and torch.equal(r64["x"], r64["u"])
    for k in ("u", "logp", "dmean"):
        check(got[k], r64[k], r32[k], what=k)
    want_logp = torch.full((n,), -(2.0 + -20.0) - LN_2PI, dtype=F64)                 # with the CLAMPED log_std
    check(got["logp"], want_logp, r32["logp"], what="logp by hand")
    g = fused.grad[t:t + 2].cpu()
    g64, g32 = r64["grad"]["log_std_parameter"], r32["grad"]["log_std_parameter"]
    print(f"log_std {log_std}: dL/dlog_std fused {g.tolist()} float64 {g64.tolist()} torch fp32 {g32.tolist()}")
    check(fused.unvector(fused.grad)["policy"], r64["grad"], r32["grad"], what="policy grad ")
    if log_std == ON_BOUNDS:
        assert torch.allclose(g64.cpu(), torch.full((2,), -alpha, dtype=F64), rtol=1e-9, atol=0)
        for c in range(2):
            check(g[c:c + 1], g64[c:c + 1], g32[c:c + 1], what=f"log_std grad[{c}]")
        for v, b in zip((fused.params, fused.adam_m, fused.adam_v), before):
            assert bool((v[t:t + 2] != b).all())                                     # both moved under Adam
    else:
        assert g.tolist() == [0.0, 0.0] and g64.tolist() == [0.0, 0.0]
        for v, b in zip((fused.params, fused.adam_m, fused.adam_v), before):
            assert torch.equal(v[t:t + 2].view(torch.int32), b.view(torch.int32))    # parameters and both moments bit-unchanged
    assert fused.stats()["actor_step"] == 1


# ---------------------------------------------------------------------------------------------------------------- NaN
def test_a_nan_draw_stays_in_its_row():
    """Both clamps keep a NaN, as torch.clamp does (rover_sac.h): a NaN in eps[r, 0] makes y[r] NaN, one in eps[r, 3] makes u[r, 1],
    logp[r] and dL/dmu[r] NaN, and no other row changes by a bit.  The statistics that average over the rows are NaN; torch's
    are too.  Rows 0, 5 / 22 / 40 / 55 lie in the four 16-row quarters of a wave's 64-row tile, row 69 in the ragged second tile.
    The two steps run on fresh trainers each: after a critic step with a NaN row the critics' weights are NaN."""
    n, rows_c, rows_p = 70, [5, 22, 69], [0, 40, 55]
    mem = memory(84)
    mods = hp_modules("nan", 83)
    idx, clean = batch(mem, n, 85)
    eps = clean.clone()
    eps[rows_c, 0] = float("nan")
    eps[rows_p, 3] = float("nan")
    nan_c, nan_p = torch.zeros(n, dtype=torch.bool, device=DEV), torch.zeros(n, dtype=torch.bool, device=DEV)
    nan_c[rows_c], nan_p[rows_p] = True, True

    def critic(e):
        f = trainers(mods)[0]
        y = torch.empty(n, device=DEV)
        f.critic_step(mem, idx, e, y_out=y)
        return {"y": y}, f.stats()

    def policy(e):
        f = trainers(mods)[0]
        out = {"u": torch.empty(n, 2, device=DEV), "logp": torch.empty(n, device=DEV), "dmean": torch.empty(n, 2, device=DEV)}
        f.policy_step(mem, idx, e, u_out=out["u"], logp_out=out["logp"], dmean_out=out["dmean"])
        return out, f.stats()

    for step, where, nan_stats, finite_stats in ((critic, nan_c, ("critic_loss", "y_mean"), ("q1_mean", "q2_mean")),
                                                 (policy, nan_p, ("policy_loss", "logp_mean", "entropy_loss"), ("alpha",))):
        got, st = step(eps)
        want, st_clean = step(clean)
        for k, v in got.items():
            assert bool(torch.isfinite(want[k]).all()), k
            assert torch.equal(torch.isnan(v).reshape(n, -1).any(1), where), k
            assert torch.equal(v[~where].view(torch.int32), want[k][~where].view(torch.int32)), k
        for k in nan_stats:
            assert math.isnan(st[k]) and math.isfinite(st_clean[k]), k
        for k in finite_stats:
            assert st[k] == st_clean[k] and math.isfinite(st[k]), k
    # the component the NaN draw does not reach
    got, want = policy(eps)[0], policy(clean)[0]
    assert bool(torch.isnan(got["u"][rows_p, 1]).all()) and torch.equal(got["u"][:, 0], want["u"][:, 0])
    assert bool(torch.isnan(got["dmean"][rows_p, 1]).all())
    # torch's statistics on the same draws, fp32
    s32 = specs(mods)[F32]
    st = s32.critic_step(*sample(mem, idx, F32), eps[:, 0:2])
    assert math.isnan(st["critic_loss"]) and math.isnan(st["y_mean"]) and math.isfinite(st["q1_mean"]) and math.isfinite(st["q2_mean"])
    assert torch.equal(torch.isnan(st["y"]).reshape(-1), nan_c)
    st = specs(mods)[F32].policy_step(sample(mem, idx, F32)[0], eps[:, 2:4])
    assert all(math.isnan(st[k]) for k in ("policy_loss", "logp_mean", "entropy_loss")) and math.isfinite(st["alpha"])


# ---------------------------------------------------------------------------------------------------------------- rows
# seeds (networks seed, memory seed + 1, batch seed + 2), picked as test_gpu_sac_hparams_edges.py picks a single step's: float64
# margins of 2.42e-4 and 1.32e-7 (hidden) with all rows terminated, 1.61e-4 and 1.39e-7 with none
TERMINATED_SEEDS = {True: 13, False: 9}


@pytest.mark.parametrize("terminated", [True, False])
def test_all_rows_or_no_rows_terminated(terminated):
    seed = TERMINATED_SEEDS[terminated]
    mem = memory(seed + 1)
    mem.terminated.fill_(terminated)
    fused, sp = trainers(hp_modules("terminated", seed))
    idx, eps = batch(mem, 512, seed + 2)
    margin, got, r64, _ = full_step(mem, fused, sp, idx, eps)
    print(f"terminated {terminated}: margin {margin:.3e} hidden {got['hidden']:.3e}")
    assert margin >= MARGIN and got["hidden"] >= HIDDEN, (margin, got["hidden"])
    r = mem.gather(idx)[2].reshape(-1)
    if terminated:
        assert torch.equal(got["y"], r)                            # y = r + (gamma * 0) * (...), bit for bit
    else:
        assert not bool((got["y"] == r).any()) and not bool((r64["critic"][0] == r.double()).any())


def test_one_row_repeated_gives_that_rows_gradients():
    """The mean over 70 copies of a row is the row: float64 runs the row once, torch fp32 the 70 copies the kernels get."""
    mem = memory(91)
    fused, sp = trainers(hp_modules("repeated", 90))
    one, e1 = batch(mem, 1, 92)
    idx, eps = one.repeat(70), e1.repeat(70, 1).contiguous()
    y = torch.empty(70, device=DEV)
    fused.critic_step(mem, idx, eps, y_out=y)
    g = fused.unvector(fused.grad)
    st = fused.stats()
    ref = {}
    for dt, rows, e in ((F64, one, e1), (F32, idx, eps)):
        s = sp[dt].critic_step(*sample(mem, rows, dt), e[:, 0:2])
        ref[dt] = {"y": s["y"].reshape(-1).expand(70), "critic_1": grads(sp[dt].critic_1), "critic_2": grads(sp[dt].critic_2), "stats": s}
    for k in ("y", "critic_1", "critic_2"):
        check(y if k == "y" else g[k], ref[F64][k], ref[F32][k], what=f"{k} ")
    for k in ("critic_loss", "q1_mean", "q2_mean", "y_mean"):
        print(f"{k}: fused {st[k]!r} float64 {ref[F64]['stats'][k]!r} torch fp32 {ref[F32]['stats'][k]!r}")
        assert abs(ref[F64]["stats"][k]) > 1e-3 and st[k] == pytest.approx(ref[F64]["stats"][k], rel=1e-3, abs=1e-6), k


# ---------------------------------------------------------------------------------------------------------------- bad_index
def one_step(fused, mem, idx, eps, step):
    n = idx.numel()
    if step == "critic":
        out = [torch.empty(n, device=DEV)]
        fused.critic_step(mem, idx, eps, y_out=out[0])
    else:
        out = [torch.empty(n, 2, device=DEV), torch.empty(n, device=DEV), torch.empty(n, 2, device=DEV)]
        fused.policy_step(mem, idx, eps, u_out=out[0], logp_out=out[1], dmean_out=out[2])
    return out


@pytest.mark.parametrize("step", ["critic", "policy"])
@pytest.mark.parametrize("bad", ["minus_one", "len", "two_to_40", "ring_pos_minus_one", "ring_pos_slots"])
def test_bad_index_is_flagged_sticky_and_reads_row_0(bad, step):
    N, n, slot = 64, 300, 2
    mem = memory(41, N=N)
    mods = hp_modules("bad_index", 40)
    fused, clean = trainers(mods)[0], trainers(mods)[0]
    ok, eps = batch(mem, n, 42)
    assert bool((ok // N == slot).any())
    idx, pos = ok.clone(), mem.ring_pos.clone()
    if bad.startswith("ring_pos"):
        mem.ring_pos[slot] = -1 if bad == "ring_pos_minus_one" else mem.slots
        out = one_step(fused, mem, idx, eps, step)
        mem.ring_pos[slot] = 0                                     # the documented substitution: ring position 0
    else:
        where = torch.tensor([0, 137, n - 1], device=DEV)
        idx[where] = {"minus_one": -1, "len": len(mem), "two_to_40": 2 ** 40}[bad]
        out = one_step(fused, mem, idx, eps, step)
        ok[where] = 0                                              # the documented substitution: row 0
    want = one_step(clean, mem, ok, eps, step)
    assert fused.stats()["bad_index"] == 1 and clean.stats()["bad_index"] == 0
    for x, y in zip(out, want):
        assert bool(torch.isfinite(y).all()) and torch.equal(x, y)
    assert_same_trainer(fused, clean, skip_state_words=(BAD_INDEX_WORD,))
    # sticky: later clean steps and a whole clean update leave the flag up, and the parameters stay finite
    mem.ring_pos.copy_(pos)
    good, eps2 = batch(mem, n, 44)
    one_step(fused, mem, good, eps2, step)
    assert fused.stats()["bad_index"] == 1
    fused.update(mem, good, eps2)
    assert fused.stats()["bad_index"] == 1 and bool(torch.isfinite(fused.params).all())
    fused.state.zero_()
    one_step(fused, mem, good, eps2, step)
    st = fused.stats()
    assert st["bad_index"] == 0 and st["critic_step" if step == "critic" else "actor_step"] == 1


# ---------------------------------------------------------------------------------------------------------------- outputs, stream
def both(seed, n=300):
    mem = memory(seed + 1)
    mods = hp_modules("both", seed)
    return (mem, trainers(mods)[0], trainers(mods)[0], *batch(mem, n, seed + 2))


def test_null_outputs_change_nothing():
    mem, a, b, idx, eps = both(52)
    n = idx.numel()
    nan = float("nan")
    y, u, logp, dmean = (torch.full(s, nan, device=DEV) for s in ((n,), (n, 2), (n,), (n, 2)))
    a.critic_step(mem, idx, eps, y_out=y)
    a.policy_step(mem, idx, eps, u_out=u, logp_out=logp, dmean_out=dmean)
    b.critic_step(mem, idx, eps)
    b.policy_step(mem, idx, eps)
    assert all(bool(torch.isfinite(x).all()) for x in (y, u, logp, dmean))
    assert_same_trainer(a, b)
    # ... and each output alone
    c = trainers(hp_modules("both", 52))[0]
    c.critic_step(mem, idx, eps)
    c.policy_step(mem, idx, eps, logp_out=torch.empty(n, device=DEV))
    assert_same_trainer(a, c)


def test_update_on_a_side_stream_is_bit_identical():
    mem, a, b, idx, eps = both(55)
    a.update(mem, idx, eps)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side and side != torch.cuda.default_stream()
        b.update(mem, idx, eps)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert_same_trainer(a, b)
    st = a.stats()
    assert (st["critic_step"], st["actor_step"], st["entropy_step"]) == (1, 1, 1) and bool(torch.isfinite(a.params).all())


@pytest.mark.parametrize("n_copies", [1, 3])
def test_every_replica_is_the_actor_block_and_nothing_behind_them_is_written(n_copies):
    mem = memory(58)
    fused = trainers(hp_modules("replicas", 57), n_copies=n_copies)[0]
    idx, eps = batch(mem, 70, 59)
    count = n_copies * fused.n_a
    assert fused.rep_a.numel() == count
    buf = torch.cat([torch.full((count,), 7.0, device=DEV), torch.full((64,), float("nan"), device=DEV)])
    fused.rep_a = buf[:count]                                       # stale replicas, a NaN guard block behind the last one
    assert fused.rep_a.data_ptr() % 16 == 0
    before = fused.params[:fused.n_a].clone()
    fused.policy_step(mem, idx, eps)
    assert not torch.equal(fused.params[:fused.n_a], before)
    rep = buf[:count].view(n_copies, -1)
    for c in range(n_copies):
        assert torch.equal(rep[c].view(torch.int32), fused.params[:fused.n_a].view(torch.int32)), c
    assert bool(torch.isnan(buf[count:]).all())
