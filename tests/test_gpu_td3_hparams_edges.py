"""Fused TD3 (include/rover_td3.h) away from its defaults and at its kernels' own edges, against the float64 torch spec by
td3_helpers.check (fused error <= 4x torch fp32's error on the same inputs, plus 1e-5 of the reference's norm); state scalars
by test_gpu_td3_update.check_critic's rule (rel 1e-3, abs 1e-6 against float64).

  A  every hyper-parameter moved, one group at a time and all together: single steps, Polyak, 20 steps, the Adam scalars;
  B  row counts around one MFMA tile (16), one reduction block (256), one weight-gradient chunk (512) and past 256 reduction
     blocks (65537, 70001), with all five statistics;
  C  a workspace that is larger than the step needs and full of NaNs, and a small step after a large one: bit for bit the
     result of a fresh, exactly sized workspace (fused against fused on purpose: every run is also covered by B).

The rewards get a mean of 1: with the zero-mean rewards of td3_helpers.fill, y_mean and the Q means are sums of terms that
cancel, and a reduction that drops rows would stay inside the statistics' tolerance."""
import numpy as np
import pytest
import torch

from td3_helpers import assert_same_trainer, check, clone_trainer, fill, nets, poison_ws, trainers
from test_gpu_td3_update import DEV, grads, params, sample, setup

pytestmark = pytest.mark.gpu

STATS = ("y_mean", "q1_mean", "q2_mean", "critic_loss", "policy_loss")
NETS = (("policy", "target_policy"), ("critic_1", "target_critic_1"), ("critic_2", "target_critic_2"))


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def shifted(mem, by=1.0):
    mem.rewards += by
    return mem


def check_stats(fused, st64, st32, keys=STATS, what=""):
    st = fused.stats()
    for k in keys:
        print(f"{what}{k}: fused {st[k]!r} float64 {st64[k]!r} torch fp32 {st32[k]!r}")
    for k in keys:
        assert abs(st64[k]) > 1e-3, (what, k, st64[k])              # the relative bound decides, not the absolute one
        assert st[k] == pytest.approx(st64[k], rel=1e-3, abs=1e-6), (what, k, st32[k])
    return st


def full_step(mem, fused, specs, idx, noise=None):
    """A critic step then an actor step on both paths.  Checks y, dL/da, the gradients of all three networks, the parameters
    after Adam and the five statistics; returns the fused values and both references."""
    n = idx.numel()
    y, dact = torch.empty(n, device=DEV), torch.empty(n, 2, device=DEV)
    fused.critic_step(mem, idx, noise, y_out=y)
    gc = fused.unvector(fused.grad)
    fused.actor_step(mem, idx, dact_out=dact)
    got = {"y": y, "dact": dact, "critic_1": gc["critic_1"], "critic_2": gc["critic_2"], "policy": fused.unvector(fused.grad)["policy"]}
    ref = {}
    for dt, sp in specs.items():
        smp = sample(mem, idx, dt)
        st = sp.critic_step(*smp, noise=None if noise is None else noise.to(dt))
        g1, g2 = grads(sp.critic_1), grads(sp.critic_2)
        a = sp.policy(smp[0]).detach().requires_grad_(True)
        da = torch.autograd.grad(-sp.critic_1(smp[0], a).mean(), a)[0]
        st.update(sp.actor_step(smp[0]))
        ref[dt] = {"y": st.pop("y").reshape(-1), "dact": da, "critic_1": g1, "critic_2": g2, "policy": grads(sp.policy), "stats": st}
    r64, r32 = ref[torch.float64], ref[torch.float32]
    for k in ("y", "dact"):
        check(got[k], r64[k], r32[k], what=f"n={n} {k}")
    for k in ("critic_1", "critic_2", "policy"):
        check(got[k], r64[k], r32[k], what=f"n={n} grad {k} ")
    p = fused.unvector(fused.params)
    for k, _ in NETS:
        check(p[k], params(getattr(specs[torch.float64], k)), params(getattr(specs[torch.float32], k)), what=f"n={n} {k} ")
    st = check_stats(fused, r64["stats"], r32["stats"], what=f"n={n} ")
    assert st["critic_step"] == 1 and st["actor_step"] == 1 and st["critic_updates"] == 1 and st["bad_index"] == 0
    return got, r64, r32


def check_targets(fused, specs, what=""):
    t = fused.unvector(fused.target)
    for _, tk in NETS:
        check(t[tk.replace("target_", "")], params(getattr(specs[torch.float64], tk)), params(getattr(specs[torch.float32], tk)),
              what=f"{what}{tk} ")


# ---------------------------------------------------------------------------------------------------------------- A
# The actor's last bias puts pi(s) near (0.55, -0.15): with noise of sigma 0.3 clipped to +-0.2 the smoothed action crosses
# act_max = 0.7 in its first component and act_min = -0.3 in its second, and stays inside on other rows.
BIAS = (0.55, -0.15)
CLAMPS = dict(noise_clip=0.2, act_min=-0.3, act_max=0.7)
HP_CASES = {
    "actor_lr_10x": dict(actor_lr=1e-3, critic_lr=1e-4),
    "critic_lr_100x": dict(actor_lr=1e-5, critic_lr=1e-3),
    "gamma_0.9": dict(gamma=0.9),
    "gamma_0": dict(gamma=0.0),
    "clamps": dict(CLAMPS),
    "adam": dict(beta1=0.8, beta2=0.99, eps=1e-4),
    "all": dict(actor_lr=1e-3, critic_lr=2e-5, gamma=0.9, polyak=0.05, beta1=0.8, beta2=0.99, eps=1e-4, **CLAMPS),
}


def hp_setup(case, seed, M=4, N=64, steps=6):
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    mods = nets(seed, DEV)
    with torch.no_grad():
        mods[0].mlp[6].bias.copy_(torch.tensor(BIAS))
    mem = ReplayMemory(M, N, device=DEV)
    fill(mem, steps, seed=seed + 1)
    fused, specs = trainers(mods, policy_delay=2, **HP_CASES[case])
    return shifted(mem), fused, specs


def assert_clamps_are_hit(spec64, mem, idx, noise, hp):
    """On the float64 spec: the noise passes both clip sides, the smoothed action both bounds, and some rows neither."""
    clip, lo, hi = (float(np.float32(hp[k])) for k in ("noise_clip", "act_min", "act_max"))
    with torch.no_grad():
        z = spec64.target_policy(mem.gather(idx)[3].double()) + noise.double().clamp(-clip, clip)
    assert bool((noise > clip).any()) and bool((noise < -clip).any())
    assert bool((z > hi).any()) and bool((z < lo).any()) and bool(((z > lo) & (z < hi)).all(1).any())
    # ... and neither symmetric bounds nor the default clip of 0.5 would give the same actions
    assert bool((z.clamp(lo, hi) != z.clamp(-hi, hi)).any()) and bool((z.clamp(lo, hi) != z.clamp(lo, -lo)).any())
    with torch.no_grad():
        z05 = spec64.target_policy(mem.gather(idx)[3].double()) + noise.double().clamp(-0.5, 0.5)
    assert bool((z.clamp(lo, hi) != z05.clamp(lo, hi)).any())


@pytest.mark.parametrize("case", list(HP_CASES))
def test_single_steps_and_polyak_with_moved_hparams(case):
    hp = HP_CASES[case]
    mem, fused, specs = hp_setup(case, seed=20)
    n = 512
    idx = mem.sample_indices(n, gen(21))
    noise = torch.randn(n, 2, device=DEV, generator=gen(22)) * 0.3
    if "noise_clip" in hp:
        assert_clamps_are_hit(specs[torch.float64], mem, idx, noise, hp)
    got, _, _ = full_step(mem, fused, specs, idx, noise)
    if hp.get("gamma") == 0.0:
        assert torch.equal(got["y"], mem.gather(idx)[2].reshape(-1))          # y = r + (0 * !terminated) * min(...) = r
    assert not torch.equal(fused.target, fused.params)
    fused.polyak()
    for sp in specs.values():
        sp.polyak()
    check_targets(fused, specs)


@pytest.mark.parametrize("case", list(HP_CASES))
def test_twenty_steps_with_moved_hparams_and_the_adam_scalars(case):
    hp = HP_CASES[case]
    mem, fused, specs = hp_setup(case, seed=23, M=5, steps=8)
    g = gen(24)
    n = 384
    for step in range(20):
        idx = mem.sample_indices(n, g)
        noise = torch.randn(n, 2, device=DEV, generator=g) * 0.3 if step % 3 == 0 else None
        stepped = fused.update(mem, idx, noise)
        last = {dt: sp.update(mem, idx, noise) for dt, sp in specs.items()}
        assert all(v["actor_stepped"] == stepped for v in last.values()) and stepped == (step % 2 == 1)
    p = fused.unvector(fused.params)
    for k, _ in NETS:
        check(p[k], params(getattr(specs[torch.float64], k)), params(getattr(specs[torch.float32], k)), what=f"{k} ")
    check_targets(fused, specs)
    st = check_stats(fused, last[torch.float64], last[torch.float32], keys=("critic_loss", "policy_loss"))
    assert st["critic_step"] == 20 and st["actor_step"] == 10 and st["critic_updates"] == 20 and st["bad_index"] == 0
    # the scalars Adam reads, in float64 from the float32 hyper-parameters and cast to float; the device's double pow and
    # sqrt may be an ulp of double off, which moves the float result by at most one float ulp (1.2e-7 relative)
    h = {k: float(getattr(fused.hp, k)) for k in ("actor_lr", "critic_lr", "beta1", "beta2")}
    for who, t in (("critic", 20), ("actor", 10)):
        size = float(np.float32(h[f"{who}_lr"] / (1.0 - h["beta1"] ** t)))
        bc2 = float(np.float32(np.sqrt(1.0 - h["beta2"] ** t)))
        print(f"{who}: step_size {st[f'{who}_step_size']!r} want {size!r}; bc2_sqrt {st[f'{who}_bc2_sqrt']!r} want {bc2!r}")
        assert st[f"{who}_step_size"] == pytest.approx(size, rel=2.5e-7, abs=0)
        assert st[f"{who}_bc2_sqrt"] == pytest.approx(bc2, rel=2.5e-7, abs=0)
    if "actor_lr" in hp:
        assert st["actor_step_size"] != st["critic_step_size"]


# ---------------------------------------------------------------------------------------------------------------- B
# Sampling is with replacement, so a memory of 4400 rows serves every n.  The workspace of n = 70001 is about 2.2 GB
# (rover_td3_workspace_bytes: 10 x 696 floats per row for the five networks' activations and their gradients, plus 137
# weight-gradient chunk partials of both critics); the float64 spec's autograd graph on the same rows is about as large.
@pytest.mark.parametrize("n", [15, 16, 17, 255, 257, 511, 513, 1025, 1026, 1027, 65537, 70001])
def test_row_counts_with_statistics(n):
    mem, fused, specs = setup(seed=30, M=4, N=1100, steps=5)
    full_step(shifted(mem), fused, specs, mem.sample_indices(n, gen(n)))


# ---------------------------------------------------------------------------------------------------------------- C
def stepped(fused, mem, idx, noise, poison_rows=0):
    """critic step, actor step, Polyak; with poison_rows the workspace is regrown and NaN-filled before each step."""
    n = idx.numel()
    y, dact = torch.empty(n, device=DEV), torch.empty(n, 2, device=DEV)
    if poison_rows:
        poison_ws(fused, poison_rows)
    fused.critic_step(mem, idx, noise, y_out=y)
    if poison_rows:
        poison_ws(fused, poison_rows)
    fused.actor_step(mem, idx, dact_out=dact)
    fused.polyak()
    return y, dact


@pytest.mark.parametrize("n", [1, 17, 300, 513])
def test_oversized_workspace_full_of_nans_changes_nothing(n):
    from isaac_rover_orbit_amd import _lib
    mem, fresh, _ = setup(seed=31)
    _, dirty, _ = setup(seed=31)
    assert_same_trainer(fresh, dirty)
    idx = mem.sample_indices(n, gen(100 + n))
    noise = torch.randn(n, 2, device=DEV, generator=gen(200 + n))
    big = 2048
    a, b = stepped(fresh, mem, idx, noise), stepped(dirty, mem, idx, noise, poison_rows=big)
    need = _lib.load().rover_td3_workspace_bytes
    assert fresh.ws.numel() == need(n) and dirty.ws.numel() == need(big) > need(n)
    assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all()) and bool(torch.isfinite(fresh.params).all())
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert_same_trainer(fresh, dirty)


@pytest.mark.parametrize("large,small", [(1000, 17), (4097, 513), (600, 1)])
def test_small_step_after_large_step_reads_only_what_it_wrote(large, small):
    mem, one, _ = setup(seed=32, M=4, N=128, steps=6)
    _, two, _ = setup(seed=32, M=4, N=128, steps=6)
    g = gen(33)
    stepped(one, mem, mem.sample_indices(large, g), torch.randn(large, 2, device=DEV, generator=g))
    clone_trainer(one, two)                      # the same starting state, but a workspace that never saw the large step
    idx = mem.sample_indices(small, g)
    noise = torch.randn(small, 2, device=DEV, generator=g)
    a, b = stepped(one, mem, idx, noise), stepped(two, mem, idx, noise)
    assert one.ws.numel() > two.ws.numel()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert_same_trainer(one, two)
    assert one.stats()["critic_step"] == 2 and one.stats()["actor_step"] == 2
