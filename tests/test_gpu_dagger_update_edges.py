"""The fused DAgger update (include/rover_dagger.h, csrc/dagger_kernels.hip) away from its defaults and at its kernels' own edges.

Bounds, none fitted to the kernel's output:
  * dz, gradients and parameters: td3_helpers.check through test_gpu_dagger.check_update (the fused error against the float64 spec
    within 4x torch fp32's error on the same inputs, plus 1e-5 of the reference's norm);
  * loss and grad_norm: check_update's rel 1e-3 / abs 1e-6 against float64, with test_gpu_td3_hparams_edges.check_stats' condition
    that the float64 value exceeds 1e-3, so the relative bound decides (dagger_helpers.strict_update);
  * step_size and bc2_sqrt: rel 2.5e-7 against float64 formed from the float32 hyper-parameters, the one-ulp bound the TD3 and SAC
    pins use for the same device code;
  * the end-row loss: loss * 2n against float64 at rel 1e-3, abs 0; a missing or doubled end row moves it by a half;
  * the clipped gradient's norm: 32 roundings of fp32 (TIGHT_TOL below);
  * everything else on the bits.

  A  hyper-parameters moved (lr, Adam, a loose and a tight clip, all together): one step at 512 rows, 20 steps at 384, the Adam
     scalars, clip_coef exactly 1 on the loose side;
  B  rows whose loss only the first and the last sampled row make, at 257, 513, 1025 and 65537 rows (a second loss block, a second
     and a third chunk, 257 block partials); plain row counts 255, 256, 1024, 1025, 1537;
  C  a memory not yet filled and one wrapped twice; a ring position outside [0, slots); an index outside the filled rows whose
     label the buffer holds;
  D  labels outside [-1, 1], a nearly saturated output, a NaN label;
  E  dz_out and replicas NULL, a side stream, an oversized workspace full of NaN, a small step after a large one: bit for bit the
     plain run."""
import math
import time

import numpy as np
import pytest
import torch

import dagger_helpers as H
from td3_helpers import check, same_bits_nan_aware
from test_gpu_dagger import biteq, check_update, grads, params, same_trainer, setup

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_INDEX_WORD = 1                        # rover_dagger_state: steps, bad_index, ...
# The clipped gradient is g * c with c = max_norm / (norm + 1e-6) and norm the fp32 sum of squares: at most 13 elements per thread in
# sequence, two halving trees of 8 levels, the 64 chunk partials, the root, the sum with 1e-6, the quotient and the product: fewer
# than 32 roundings of 2**-24 each, whatever their signs.
TIGHT_TOL = 32 * 2.0 ** -24


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def D():
    from isaac_rover_orbit_amd import dagger
    return dagger


# ---------------------------------------------------------------------------------------------------------------- A
ADAM = dict(beta1=0.8, beta2=0.99, eps=1e-4)
HP_CASES = {
    "lr": dict(learning_rate=1e-2),
    "adam": dict(ADAM),
    "clip_loose": dict(grad_norm_clip="loose"),
    "clip_tight": dict(grad_norm_clip=1e-3),
    "all": dict(learning_rate=1e-2, grad_norm_clip=1e-3, **ADAM),
}


def hp_setup(case, seed, idx_of, **kw):
    """setup() under HP_CASES[case], and the batch.  The loose clip is ten times the float64 reference's grad_norm on that batch,
    from a student of the same seed before the trainer under test exists."""
    hp = dict(HP_CASES[case])
    mem, _, specs = setup(seed=seed, **kw)
    idx = idx_of(mem)
    norm = H.reference_scalars(specs[torch.float64], mem, idx)["grad_norm"]
    if hp.get("grad_norm_clip") == "loose":
        hp["grad_norm_clip"] = 10.0 * norm
    mem2, fused, specs = setup(seed=seed, **kw, **hp)
    assert biteq(mem2.obs, mem.obs) and biteq(mem2.actions, mem.actions)
    return mem2, fused, specs, idx, hp, norm


@pytest.mark.parametrize("case", list(HP_CASES))
def test_single_step_with_moved_hparams(case):
    mem, fused, specs, idx, hp, norm = hp_setup(case, 20, lambda m: m.sample_indices(512, gen(21)))
    st, _, want = H.strict_update(mem, fused, specs, idx)
    if case == "clip_loose":
        assert st["clip_coef"] == 1.0                                      # min(1, 10 norm / (norm + 1e-6)): the gradient is left alone
        _, plain, _ = setup(seed=20)
        plain.update(mem, idx)
        same_trainer(fused, plain)
    if case in ("clip_tight", "all"):
        clipped = float(fused.grad.double().norm())
        lower = 1e-3 * want["grad_norm"] / (want["grad_norm"] + 1e-6)
        print(f"{case}: |clipped gradient| {clipped!r}, clip {fused.hp.grad_norm_clip!r}, clip_coef {st['clip_coef']!r}")
        assert st["clip_coef"] < 1.0 and lower * (1 - 1e-3) <= clipped <= float(fused.hp.grad_norm_clip) * (1 + TIGHT_TOL)


@pytest.mark.parametrize("case", list(HP_CASES))
def test_twenty_steps_with_moved_hparams_and_the_adam_scalars(case):
    """Every one of the 20 steps is held to float64 from where the fused trainer stands (dagger_helpers.reference_at): the gradient by
    check, loss and grad_norm by strict_update's rule, and Adam's element by adam_step_float64's bound, which pins beta1, beta2 and eps
    (the first step of a bias-corrected Adam does not depend on the betas).  At the default learning rate the parameters after the 20
    steps also pass check against the float64 and float32 specs that ran beside the fused trainer.  At lr = 1e-2 that comparison is
    not made: weights of size 0.03 move by up to 0.2 and the trajectory is unstable.  Measured on the MI355X over three seeds: a
    float64 spec started 1e-7 (relative) away from the reference ends 9e-5 to 0.23 away from it, a float32 torch spec started one ulp
    away 7e-5 to 2.4, the fused trainer 0.04 to 0.10, of a parameter norm of 24.5."""
    g = gen(24)
    mem, fused, specs, _, hp, _ = hp_setup(case, 23, lambda m: m.sample_indices(384, gen(25)), M=5, steps=8)
    h = {k: float(getattr(fused.hp, k)) for k in ("lr", "beta1", "beta2", "eps", "grad_norm_clip")}
    n_a = fused.n_a
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for step in range(1, 21):
        idx = mem.sample_indices(384, g)
        ref = H.reference_at(fused, specs, mem, idx)
        before = [getattr(fused, k)[:n_a].double() for k in ("params", "adam_m", "adam_v")]
        fused.update(mem, idx)
        last = {dt: sp.update(mem, idx) for dt, sp in specs.items()}
        st = fused.stats()
        (loss64, norm64, g64), (_, norm32, g32) = ref[torch.float64], ref[torch.float32]
        for k, want in (("loss", loss64), ("grad_norm", norm64)):
            assert want > 1e-3 and st[k] == pytest.approx(want, rel=1e-3, abs=1e-6), (step, k, st[k], want)
        c64, c32 = (min(1.0, h["grad_norm_clip"] / (x + 1e-6)) if h["grad_norm_clip"] > 0 else 1.0 for x in (norm64, norm32))
        check(fused.unvector(fused.grad)["policy"], {k: v * c64 for k, v in g64.items()}, {k: v * c32 for k, v in g32.items()},
              what=f"step {step} grad ")
        wants = H.adam_step_float64(*before[:1], fused.grad[:n_a].double(), *before[1:], step, h["lr"], h["beta1"], h["beta2"], h["eps"])
        for name, vec, (want, tol) in zip(("p", "m", "v"), (fused.params, fused.adam_m, fused.adam_v), wants):
            ratio = float(((vec[:n_a].double() - want).abs() / tol).max())
            worst[name] = max(worst[name], ratio)
            assert ratio <= 1.0, (step, name, ratio)
        assert st["steps"] == step and st["bad_index"] == 0
        if case == "clip_loose":
            assert st["clip_coef"] == 1.0
    print(f"{case}: the largest |fused - float64 Adam| / bound over 20 steps: {worst}")
    r64 = last[torch.float64]
    print(f"{case}: loss fused {st['loss']!r} float64 spec {r64['loss']!r}; grad_norm fused {st['grad_norm']!r} float64 spec {r64['grad_norm']!r}")
    if "learning_rate" not in hp:
        check(fused.unvector(fused.params)["policy"], params(specs[torch.float64]), params(specs[torch.float32]), what="params ")
        for k in ("loss", "grad_norm"):
            assert r64[k] > 1e-3 and st[k] == pytest.approx(r64[k], rel=1e-3, abs=1e-6), k
    # the scalars Adam reads, in float64 from the float32 hyper-parameters and cast to float
    size = float(np.float32(h["lr"] / (1.0 - h["beta1"] ** 20)))
    bc2 = float(np.float32(np.sqrt(1.0 - h["beta2"] ** 20)))
    print(f"{case}: step_size {st['step_size']!r} want {size!r}; bc2_sqrt {st['bc2_sqrt']!r} want {bc2!r}")
    assert st["step_size"] == pytest.approx(size, rel=2.5e-7, abs=0) and st["bc2_sqrt"] == pytest.approx(bc2, rel=2.5e-7, abs=0)
    if "learning_rate" in hp:
        assert h["lr"] == H.f32(1e-2)
    if "beta1" in hp:
        assert (h["beta1"], h["beta2"], h["eps"]) == (H.f32(0.8), H.f32(0.99), H.f32(1e-4))


# ---------------------------------------------------------------------------------------------------------------- B
K_STAR = 1234


@pytest.fixture(scope="module")
def end_rows():
    """A memory of 4400 rows whose labels are the fused student's own inference output, except row K_STAR: that label is the output
    plus (0.5, -0.5).  Shared by the end-row cases and left unchanged: every case builds its own trainer from the same seed."""
    mem, fused, _ = setup(seed=30, M=4, N=1100, steps=5)
    rows = mem.gather(torch.arange(len(mem), device=DEV))[0]
    labels = fused.actor(rows.contiguous()).clone()
    labels[K_STAR] += torch.tensor([0.5, -0.5], device=DEV)
    mem.actions.view(-1, 2).copy_(labels)
    return mem


def end_row_case(mem, n):
    _, fused, specs = setup(seed=30, M=1, N=1, steps=1)                     # the same student; its own memory is not used
    other = torch.randint(0, len(mem) - 1, (n,), device=DEV, generator=gen(n))
    idx = other + (other >= K_STAR)
    idx[0] = idx[n - 1] = K_STAR
    assert int((idx == K_STAR).sum()) == 2
    want = H.reference_scalars(specs[torch.float64], mem, idx)
    d2 = want["d2"]
    rest = float(d2.sum() - d2[0] - d2[n - 1])
    assert rest < 1e-6 * float(d2.sum()) and float(d2[0]) == pytest.approx(0.5, rel=1e-4) and float(d2[n - 1]) == pytest.approx(float(d2[0]), rel=1e-9)
    assert want["loss"] * 2 * n == pytest.approx(1.0, rel=1e-4)             # 2 * 0.5 / (2n)
    t0 = time.perf_counter()
    st, _ = check_update(mem, fused, specs, idx)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    print(f"n={n}: loss * 2n fused {st['loss'] * 2 * n!r} float64 {want['loss'] * 2 * n!r}; update and both specs {wall:.2f} s")
    assert st["loss"] * 2 * n == pytest.approx(want["loss"] * 2 * n, rel=1e-3, abs=0)


@pytest.mark.parametrize("n", [257, 513, 1025])
def test_first_and_last_row_make_the_loss(end_rows, n):
    end_row_case(end_rows, n)


def test_65537_rows_take_the_strided_reduction(end_rows):
    """257 block partials: the one-workgroup reduce adds t and t + 256 before its tree."""
    t0 = time.perf_counter()
    end_row_case(end_rows, 65537)
    print(f"65537 rows: {time.perf_counter() - t0:.2f} s in all")


@pytest.mark.parametrize("n", [255, 256, 1024, 1025, 1537])
def test_plain_row_counts(n):
    mem, fused, specs = setup(seed=n % 5, M=4, N=160, steps=5)
    H.strict_update(mem, fused, specs, mem.sample_indices(n, gen(n)))


# ---------------------------------------------------------------------------------------------------------------- C
def test_memory_not_yet_filled():
    mem, fused, specs = setup(seed=40, M=5, N=64, steps=2)                  # 2 adds into 6 slots
    assert mem.slots == 6 and not mem.filled and len(mem) == 128
    H.strict_update(mem, fused, specs, mem.sample_indices(300, gen(41)))


def test_memory_wrapped_twice():
    mem, fused, specs = setup(seed=42, M=4, N=64, steps=11)
    assert mem.filled and mem.memory_index == 3 and sorted(mem.ring_pos.tolist()) != mem.ring_pos.tolist()
    H.strict_update(mem, fused, specs, mem.sample_indices(300, gen(43)))


def same_but_the_flag(fused, clean):
    for name in ("params", "grad", "adam_m", "adam_v", "rep_a"):
        assert biteq(getattr(fused, name), getattr(clean, name)), name
    keep = [i for i in range(fused.state.numel()) if i != BAD_INDEX_WORD]
    assert torch.equal(fused.state[keep], clean.state[keep])


@pytest.mark.parametrize("bad", ["ring_pos_minus_one", "ring_pos_slots"])
def test_bad_ring_position_is_flagged_sticky_and_reads_slot_0(bad):
    """test_gpu_td3_degenerate's rule: the observation comes from ring slot 0 of the same env, the label stays the row's."""
    M, N, n, slot = 4, 64, 300, 2
    mem, fused, _ = setup(seed=44, M=M, N=N, steps=6)
    _, clean, _ = setup(seed=44, M=M, N=N, steps=6)
    idx = mem.sample_indices(n, gen(45))
    assert bool((idx // N == slot).any()) and int(mem.ring_pos[slot]) != 0
    pos = mem.ring_pos.clone()
    dz, want = torch.empty(n, 2, device=DEV), torch.empty(n, 2, device=DEV)
    mem.ring_pos[slot] = -1 if bad == "ring_pos_minus_one" else mem.slots
    fused.update(mem, idx, dz_out=dz)
    mem.ring_pos[slot] = 0
    clean.update(mem, idx, dz_out=want)
    assert fused.stats()["bad_index"] == 1 and clean.stats()["bad_index"] == 0
    assert bool(torch.isfinite(want).all()) and biteq(dz, want)
    same_but_the_flag(fused, clean)
    mem.ring_pos.copy_(pos)
    fused.update(mem, mem.sample_indices(n, gen(46)))
    assert fused.stats()["bad_index"] == 1                                  # sticky


def test_index_past_the_filled_rows_reads_label_0_not_the_buffer():
    """The memory holds 2 of 5 slots; the rows behind them exist in the label buffer and hold 0.9.  An index there is out of range:
    the flag goes up and the row is row 0, label included -- the loss head checks the index before it reads the label."""
    mem, fused, _ = setup(seed=47, M=5, N=64, steps=2)
    _, clean, _ = setup(seed=47, M=5, N=64, steps=2)
    valid = len(mem)
    mem.actions.view(-1, 2)[valid:] = 0.9
    n = 300
    ok = mem.sample_indices(n, gen(48))
    idx = ok.clone()
    where = torch.tensor([0, 137, 255, 256, n - 1], device=DEV)
    idx[where] = torch.tensor([valid, valid + 1, mem.memory_size * 64 - 1, valid, valid + 63], device=DEV)
    ok[where] = 0
    dz, want = torch.empty(n, 2, device=DEV), torch.empty(n, 2, device=DEV)
    fused.update(mem, idx, dz_out=dz)
    clean.update(mem, ok, dz_out=want)
    assert fused.stats()["bad_index"] == 1 and clean.stats()["bad_index"] == 0
    assert bool(torch.isfinite(want).all()) and biteq(dz, want)
    same_but_the_flag(fused, clean)


# ---------------------------------------------------------------------------------------------------------------- D
def test_labels_outside_the_unit_interval():
    mem, fused, specs = setup(seed=50)
    mem.actions.copy_(torch.rand(mem.actions.shape, device=DEV, generator=gen(51)) * 6 - 3)
    assert float(mem.actions.abs().max()) > 2.5
    H.strict_update(mem, fused, specs, mem.sample_indices(300, gen(52)))


def test_nearly_saturated_outputs():
    mem, fused, specs = setup(seed=53, bias=(4.0, -4.0))
    idx = mem.sample_indices(300, gen(54))
    out = fused.actor(mem.gather(idx)[0].contiguous())
    slope = 1 - out.double() ** 2
    assert 0 < float(slope.min()) and float(slope.max()) < 0.02             # 1 - t^2 is small but not zero
    _, dz, _ = H.strict_update(mem, fused, specs, idx, scalars=("loss",))
    assert bool((dz != 0).all())


def test_one_nan_label():
    """Column 0 of one sampled row's label is NaN: dz of that row and column is NaN, and with it every gradient the row reaches:
    all of them but the last layer's row and bias of column 1.  Asserted only where the float32 torch spec shows the same."""
    mem, fused, specs = setup(seed=55)
    idx = mem.sample_indices(300, gen(56))
    row = int(idx[77])
    mem.actions.view(-1, 2)[row, 0] = float("nan")
    dz = torch.empty(300, 2, device=DEV)
    fused.update(mem, idx, dz_out=dz)
    out = {dt: sp.update(mem, idx) for dt, sp in specs.items()}
    st = fused.stats()
    assert math.isnan(st["loss"]) and math.isnan(out[torch.float32]["loss"]) and st["bad_index"] == 0 and st["steps"] == 1
    hit = idx == row
    assert torch.equal(torch.isnan(dz), torch.isnan(out[torch.float32]["dz"])) and bool(torch.isnan(dz[hit, 0]).all())
    assert int(torch.isnan(dz).sum()) == int(hit.sum())
    for name, vec in (("grad", fused.grad), ("params", fused.params), ("adam_m", fused.adam_m), ("adam_v", fused.adam_v)):
        got = fused.unvector(vec)["policy"]
        ref32 = (grads if name == "grad" else params)(specs[torch.float32])
        ref64 = (grads if name == "grad" else params)(specs[torch.float64])
        for k in ref32:
            nan = torch.isnan(got[k])
            if name in ("grad", "params"):
                assert torch.equal(nan, torch.isnan(ref32[k].cpu())), (name, k)
                if not bool(nan.all()):                                     # what the row does not reach follows the usual rule
                    check(got[k][~nan], ref64[k].cpu()[~nan], ref32[k].cpu()[~nan], what=f"{name} {k} ")
            else:
                assert torch.equal(nan, torch.isnan(fused.unvector(fused.grad)["policy"][k])), (name, k)
    finite = sum(int((~torch.isnan(v)).sum()) for v in fused.unvector(fused.params)["policy"].values())
    assert finite == 128 + 1                                               # mlp.6.weight[1] and mlp.6.bias[1]
    rep = fused.rep_a.view(fused.n_copies, -1)
    assert all(same_bits_nan_aware(rep[c], fused.params[:fused.n_a]) for c in range(fused.n_copies))


# ---------------------------------------------------------------------------------------------------------------- E
def pair(seed, n=300, **kw):
    mem, a, _ = setup(seed=seed, **kw)
    _, b, _ = setup(seed=seed, **kw)
    return mem, a, b, mem.sample_indices(n, gen(seed + 1))


def test_dz_out_null_changes_nothing():
    mem, a, b, idx = pair(60)
    dz = torch.full((300, 2), float("nan"), device=DEV)
    a.update(mem, idx, dz_out=dz)
    b.update(mem, idx)
    same_trainer(a, b)
    assert bool(torch.isfinite(dz).all())


def test_replicas_null_leaves_the_replica_buffer_alone():
    mem, a, b, idx = pair(61)
    before = b.rep_a.clone()
    H.update(a, mem, idx)                                                  # the C wrapper with the replicas: FusedDAgger.update's call
    H.update(b, mem, idx, replicas=False)
    for name in ("params", "grad", "adam_m", "adam_v", "state"):
        assert biteq(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), name
    assert biteq(b.rep_a, before) and not biteq(a.rep_a, before)
    assert biteq(a.rep_a.view(a.n_copies, -1)[a.n_copies - 1], a.params[:a.n_a])


def test_side_stream_matches_the_default_stream():
    mem, a, b, idx = pair(62)
    a.update(mem, idx)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b.update(mem, idx)
    side.synchronize()
    same_trainer(a, b)


@pytest.mark.parametrize("n", [1, 17, 300, 513])
def test_oversized_workspace_full_of_nans_changes_nothing(n):
    from isaac_rover_orbit_amd import _lib
    mem, fresh, dirty, idx = pair(63, n=n)
    need = int(_lib.load().rover_dagger_workspace_bytes(n))
    dirty.ws = torch.full((4 * need,), 0xFF, dtype=torch.uint8, device=DEV)
    fresh.update(mem, idx)
    dirty.update(mem, idx)
    assert fresh.ws.numel() == need and dirty.ws.numel() == 4 * need
    assert bool(torch.isfinite(fresh.params).all()) and bool(torch.isfinite(fresh.grad).all())
    same_trainer(fresh, dirty)


@pytest.mark.parametrize("large,small", [(1100, 513), (600, 1)])
def test_small_step_after_large_step_reads_only_what_it_wrote(large, small):
    mem, one, two, _ = pair(64, N=128)
    g = gen(65)
    one.update(mem, mem.sample_indices(large, g))
    for name in ("params", "grad", "adam_m", "adam_v", "state", "rep_a"):   # the same starting state, but a workspace that never
        getattr(two, name).copy_(getattr(one, name))                        # saw the large step
    idx = mem.sample_indices(small, g)
    one.update(mem, idx)
    two.update(mem, idx)
    assert one.ws.numel() > two.ws.numel()
    same_trainer(one, two)
    assert one.stats()["steps"] == 2
