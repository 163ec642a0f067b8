"""Fused SAC (include/rover_sac.h) away from its defaults and at its kernels' own edges, against the float64 torch spec by
td3_helpers.check (fused error <= 4x torch fp32's error on the same inputs, plus 1e-5 of the reference's norm); state scalars
by rel 1e-3, abs 1e-6 against float64, with |reference| > 1e-3 asserted so that the relative bound decides; the Adam scalars by
rel 2.5e-7 against float32(lr / (1 - beta1^t)) and float32(sqrt(1 - beta2^t)) (test_gpu_td3_hparams_edges.py has the derivation).

  A  every hyper-parameter moved, one group at a time and all together, and the entropy coefficient far from 0.2: single steps
     with Polyak, 20 updates, the six Adam scalars; then the three Adam clocks driven apart (3, 2, 1);
  B  row counts of 1 and around one MFMA tile (16), one dense block (64), one reduction block (256), one weight-gradient chunk
     (512), two chunks (1025) and past 256 reduction blocks (65537), with all eight statistics;
  C  a workspace that is larger than the step needs and full of NaNs, and a small step after a large one: bit for bit the
     result of a fresh, exactly sized workspace (fused against fused on purpose: every run is also covered by B).

The rewards get a mean of 1: with the zero-mean rewards of td3_helpers.fill, y_mean and the Q means are sums of terms that
cancel, and a reduction that drops rows would stay inside the statistics' tolerance.  The actor's last bias is (1.5, -1.5): the
mean sits near (0.9, -0.9), so x = mu + sigma eps passes +1 in the first component and -1 in the second on many rows and stays
inside on others.

Every input is made on the CPU and copied to the device, so the seeds, picked with TorchSAC in float64 on the CPU so that no
clamp (| |x| - 1 |) and no min (| q1 - q2 |) decision of a run lies within 1e-4 of flipping, no LeakyReLU' decision within
HIDDEN (see there) and no statistic of the float64 spec within 1e-3 of zero, name the same run here.  Each test asserts those
margins again.

One statistic cannot meet |reference| > 1e-3: alpha in the case alpha_tiny (exp(-10) = 4.5e-5).  alpha is a function of one
float, (float)exp((double)log_alpha), so everywhere it is held to the stricter rule of the Adam scalars, rel 2.5e-7 against
float32(exp(float64(log_alpha))), and to the statistics' rule as well wherever the reference is above 1e-3."""
import math

import numpy as np
import pytest
import torch

from sac_helpers import (HiddenMargin, assert_same_trainer, check, clone_trainer, decision_margin, draws, fill, nets, params, poison_ws, sample,
                         specs, trainers)
from test_gpu_sac_update import DEV, F32, F64, critic_case, policy_case
from test_gpu_sac_update import memory as device_memory

pytestmark = pytest.mark.gpu

CRITIC_STATS = ("critic_loss", "q1_mean", "q2_mean", "y_mean")
POLICY_STATS = ("policy_loss", "entropy_loss", "logp_mean", "alpha")
NETS = ("policy", "critic_1", "critic_2")
CLOCKS = ("critic", "actor", "entropy")
MARGIN = 1e-4
# LeakyReLU' is the third kind of decision: a hidden unit whose float64 pre-activation is closer to 0 than fp32's error on it
# takes the other slope in fp32, and one such unit moves a weight gradient by about 1e-2 of its norm.  torch fp32's rms error on
# these pre-activations is 9e-9 (128 inputs) to 9e-8 (the 965-wide first layer).  A single step's seed keeps every unit a step
# differentiates through 1e-7 from 0.  Over 20 updates of 384 rows (15 million such units) no seed can: every run has units
# within 3e-8, so those seeds keep them 2e-8 away, twice the mid layers' rms error, which is what a search can still find.
HIDDEN, HIDDEN_20 = 1e-7, 2e-8


def memory(seed, M=4, N=64, steps=6, device=DEV, shift=1.0):
    """td3_helpers.fill on the CPU with the rewards shifted; on the CPU as it is (the seed search), else copied to the device."""
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    if str(device) == "cpu":
        mem = ReplayMemory(M, N, device="cpu")
        fill(mem, steps, seed=seed)
    else:
        mem = device_memory(seed, M, N, steps)
    mem.rewards += shift
    return mem


def batch(mem, n, seed):
    """(idx, eps) of one step, drawn on the CPU from one seed and copied to the memory's device."""
    idx = torch.randint(0, len(mem), (n,), generator=torch.Generator().manual_seed(seed))
    return idx.to(mem.obs.device), draws(n, seed + 1).to(mem.obs.device)


def alpha_of(log_alpha):
    """(float)exp((double)log_alpha) of the float32 ``log_alpha``, as rover_sac.h forms the coefficient."""
    return float(np.float32(np.exp(np.float64(np.float32(log_alpha)))))


def check_stats(st, st64, st32, keys, what="", log_alpha=None):
    """The fused statistics ``st`` against the float64 spec's; ``log_alpha``: the float the last policy step read."""
    for k in keys:
        print(f"{what}{k}: fused {st[k]!r} float64 {st64[k]!r} torch fp32 {st32[k]!r}")
    for k in keys:
        if k == "alpha":
            assert st[k] == pytest.approx(alpha_of(log_alpha), rel=2.5e-7, abs=0), (what, k)
            if abs(st64[k]) <= 1e-3:                                 # alpha_tiny only, see the module's docstring
                assert st64[k] < 1e-4
                continue
        assert abs(st64[k]) > 1e-3, (what, k, st64[k])              # the relative bound decides, not the absolute one
        assert st[k] == pytest.approx(st64[k], rel=1e-3, abs=1e-6), (what, k, st32[k])


def check_params(fused, sp, nets_=NETS, what=""):
    p = fused.unvector(fused.params)
    s64, s32 = sp[F64], sp[F32]
    for k in nets_:
        check(p[k], params(getattr(s64, k)), params(getattr(s32, k)), what=f"{what}{k} ")
    check(p["log_entropy_coefficient"], s64.log_entropy_coefficient.detach().reshape(1), s32.log_entropy_coefficient.detach().reshape(1),
          what=f"{what}log_alpha")


def check_targets(fused, sp, what=""):
    t = fused.unvector(fused.target)
    for k in ("critic_1", "critic_2"):
        check(t[k], params(getattr(sp[F64], "target_" + k)), params(getattr(sp[F32], "target_" + k)), what=f"{what}target_{k} ")


def check_adam_scalars(fused, st, steps, what=""):
    """The six scalars Adam reads, in float64 from the float32 hyper-parameters and cast to float (the device's double pow and
    sqrt may be an ulp of double off, which moves the float result by at most one float ulp, 1.2e-7 relative); ``steps``: the
    (critic, actor, entropy) step counts."""
    h = {k: float(getattr(fused.hp, k)) for k in ("actor_lr", "critic_lr", "entropy_lr", "beta1", "beta2")}
    worst = 0.0
    for who, t in zip(CLOCKS, steps):
        size = float(np.float32(h[f"{who}_lr"] / (1.0 - h["beta1"] ** t)))
        bc2 = float(np.float32(np.sqrt(1.0 - h["beta2"] ** t)))
        print(f"{what}{who}: step_size {st[f'{who}_step_size']!r} want {size!r}; bc2_sqrt {st[f'{who}_bc2_sqrt']!r} want {bc2!r}")
        assert st[f"{who}_step_size"] == pytest.approx(size, rel=2.5e-7, abs=0), who
        assert st[f"{who}_bc2_sqrt"] == pytest.approx(bc2, rel=2.5e-7, abs=0), who
        worst = max(worst, abs(st[f"{who}_step_size"] / size - 1), abs(st[f"{who}_bc2_sqrt"] / bc2 - 1))
    print(f"{what}worst relative deviation of an Adam scalar: {worst:.3e}")
    for i, a in enumerate(CLOCKS):
        for j, b in enumerate(CLOCKS[:i]):
            if h[f"{a}_lr"] != h[f"{b}_lr"] and steps[i] == steps[j]:
                assert st[f"{a}_step_size"] != st[f"{b}_step_size"], (a, b)
            if steps[i] != steps[j]:
                assert st[f"{a}_bc2_sqrt"] != st[f"{b}_bc2_sqrt"], (a, b)


def full_step(mem, fused, sp, idx, eps, continuous_only=False, steps=(1, 1, 1)):
    """A critic step then a policy step on every path.  Checks y, the gradients of all three networks, log_std's gradient,
    u / logp / dL/dmu, the parameters, log_std and log_alpha after Adam and the eight statistics; with ``continuous_only`` only
    what is continuous in the clamp and min decisions: y, the critics' gradients and the statistics.  Returns the float64
    spec's decision margin, the fused values (with the float64 spec's HiddenMargin as "hidden") and both references."""
    n = idx.numel()
    s64 = sp[F64]
    smp = sample(mem, idx, F64)
    la0 = float(fused.log_alpha)
    margin = decision_margin(s64, smp[3], eps[:, 0:2], s64.target_critic_1, s64.target_critic_2)
    with HiddenMargin(s64.critic_1, s64.critic_2) as hidden_c:
        y, out = critic_case(mem, fused, sp, idx, eps)
    c64, c32 = out[F64], out[F32]
    g = fused.unvector(fused.grad)
    st = fused.stats()
    check(y, c64[0], c32[0], what=f"n={n} y")
    check(g["critic_1"], c64[1], c32[1], what=f"n={n} grad c1 ")
    check(g["critic_2"], c64[2], c32[2], what=f"n={n} grad c2 ")
    check_stats(st, c64[3], c32[3], CRITIC_STATS, what=f"n={n} ")
    if not continuous_only:
        check_params(fused, sp, ("critic_1", "critic_2"), what=f"n={n} ")
    margin = min(margin, decision_margin(s64, smp[0], eps[:, 2:4], s64.critic_1, s64.critic_2))
    with HiddenMargin(s64.policy, s64.critic_1, s64.critic_2) as hidden_p:
        got, pout = policy_case(mem, fused, sp, idx, eps)
    p64, p32 = pout[F64], pout[F32]
    st = fused.stats()
    check_stats(st, p64["stats"], p32["stats"], POLICY_STATS, what=f"n={n} ", log_alpha=la0)
    assert (st["critic_step"], st["actor_step"], st["entropy_step"], st["bad_index"]) == (*steps, 0)
    got.update(y=y, critic_1=g["critic_1"], critic_2=g["critic_2"], policy=fused.unvector(fused.grad)["policy"])
    if not continuous_only:
        for k in ("u", "logp", "dmean"):
            check(got[k], p64[k], p32[k], what=f"n={n} {k}")
        check(got["policy"], p64["grad"], p32["grad"], what=f"n={n} grad policy ")
        check_params(fused, sp, what=f"n={n} ")
    got["hidden"] = min(hidden_c.value, hidden_p.value)
    return margin, got, {"critic": c64, "policy": p64}, {"critic": c32, "policy": p32}


# ---------------------------------------------------------------------------------------------------------------- A
BIAS = (1.5, -1.5)
LOG_20 = math.log(20.0)
# log_std = (-5, 1.5) under target_entropy = +1: logp_mean is then near +1.1, between the default target's +2 and -1, so that
# logp_mean + target_entropy is positive where the default's is negative (with log_std = 0, logp_mean is near -2.3 and +1
# would not change the sign).  The second component, sigma = 4.5 around -0.9, passes both -1 and +1 and stays inside on other
# rows; the first, sigma = 0.007 around 0.9, never reaches +1: a narrow Gaussian whose mean is a fraction of a sigma from the
# clamp, such as (-1.25, -1.25), puts a row within 1e-4 of it in nearly every run of 20 updates.
NARROW = (-5.0, 1.5)
HP_CASES = {
    "actor_lr_10x": dict(actor_lr=1e-3, critic_lr=1e-4),
    "critic_lr_100x": dict(actor_lr=1e-5, critic_lr=1e-3),
    "entropy_lr": dict(entropy_lr=5e-2),
    "gamma_0.9": dict(gamma=0.9),
    "gamma_0": dict(gamma=0.0),
    "adam": dict(beta1=0.8, beta2=0.99, eps=1e-4),
    "target_entropy_+1": dict(target_entropy=1.0),
    "polyak_0.05": dict(polyak=0.05),
    "alpha_20": dict(log_entropy_coefficient=LOG_20),
    "alpha_tiny": dict(log_entropy_coefficient=-10.0),
    "all": dict(actor_lr=1e-3, critic_lr=2e-5, entropy_lr=5e-2, gamma=0.9, polyak=0.05, beta1=0.8, beta2=0.99, eps=1e-4,
                target_entropy=1.0, log_entropy_coefficient=math.log(2.0)),
}
LOG_STD = {"target_entropy_+1": NARROW, "all": NARROW}


def hp_modules(case, seed, device=DEV):
    return [m.to(device) for m in nets(seed, "cpu", bias=BIAS, log_std=LOG_STD.get(case))]


def assert_both_clamps_and_interior(spec64, states, e):
    with torch.no_grad():
        ls = spec64.policy.log_std_parameter.clamp(-20, 2)
        x = spec64.policy(states) + ls.exp() * e.double()
    assert bool((x > 1).any()) and bool((x < -1).any()) and bool((x.abs() < 1).all(1).any())


# seeds of the single steps at n = 512 (networks seed, memory seed + 1, batch seed + 2): per case the first seed from 0 on at
# which the float64 spec on the CPU has a margin >= 1.2e-4, a hidden margin >= 1.2e-7 and every statistic above 2e-3; behind
# each seed the two margins it reaches
SINGLE_SEEDS = {
    "actor_lr_10x": 1,          # 1.41e-4, 2.14e-7
    "critic_lr_100x": 1,        # 1.41e-4, 1.41e-7
    "entropy_lr": 1,            # 1.41e-4, 2.14e-7
    "gamma_0.9": 1,             # 1.41e-4, 3.26e-7
    "gamma_0": 13,              # 2.42e-4, 1.32e-7
    "adam": 9,                  # 1.61e-4, 1.39e-7
    "target_entropy_+1": 4,     # 6.69e-3, 1.84e-7
    "polyak_0.05": 1,           # 1.41e-4, 2.14e-7
    "alpha_20": 1,              # 1.41e-4, 4.14e-7
    "alpha_tiny": 1,            # 1.41e-4, 1.28e-7
    "all": 1,                   # 9.56e-4, 2.50e-7
}


@pytest.mark.parametrize("case", list(HP_CASES))
def test_single_steps_and_polyak_with_moved_hparams(case):
    hp, seed = HP_CASES[case], SINGLE_SEEDS[case]
    mem = memory(seed + 1)
    fused, sp = trainers(hp_modules(case, seed), **hp)
    n = 512
    idx, eps = batch(mem, n, seed + 2)
    smp = sample(mem, idx, F64)
    assert_both_clamps_and_interior(sp[F64], smp[3], eps[:, 0:2])
    assert_both_clamps_and_interior(sp[F64], smp[0], eps[:, 2:4])
    la0 = float(fused.log_alpha)
    margin, got, r64, _ = full_step(mem, fused, sp, idx, eps)
    print(f"{case}: margin {margin:.3e} hidden {got['hidden']:.3e}")
    assert margin >= MARGIN and got["hidden"] >= HIDDEN, (margin, got["hidden"])
    if hp.get("gamma") == 0.0:
        assert torch.equal(got["y"], mem.gather(idx)[2].reshape(-1))          # y = r + (0 * !terminated) * (...) = r
    d = r64["policy"]["stats"]["logp_mean"]
    assert d - 2.0 < 0                                                         # the default target's sign ...
    if "target_entropy" in hp:
        assert d + hp["target_entropy"] > 0                                    # ... and this one's
        assert float(fused.log_alpha) > la0                                    # log_alpha moves up where the default moves it down
    else:
        assert float(fused.log_alpha) < la0
    assert not torch.equal(fused.target, fused.params[fused.n_a:fused.n_a + 2 * fused.n_c])
    fused.polyak()
    for s in sp.values():
        s.polyak()
    check_targets(fused, sp)


# seeds of the 20 updates at n = 384 (networks seed, memory seed + 1, step i's batch 1000 * seed + 2 * i): per case the first seed
# from 0 on at which the float64 spec on the CPU keeps, over all 20 updates, a margin >= 1.2e-4 and a hidden margin >= 2.4e-8 and
# ends with every statistic above 2e-3 -- about one seed in 700; behind each seed the two margins it reaches
TWENTY_SEEDS = {
    "actor_lr_10x": 153,        # 1.46e-4, 3.20e-8
    "critic_lr_100x": 333,      # 1.20e-4, 2.98e-8
    "entropy_lr": 535,          # 1.81e-4, 2.79e-8
    "gamma_0.9": 497,           # 1.50e-4, 2.65e-8
    "gamma_0": 854,             # 1.64e-4, 3.19e-8
    "adam": 2060,               # 1.23e-4, 2.84e-8
    "target_entropy_+1": 16,    # 4.43e-4, 2.46e-8
    "polyak_0.05": 2734,        # 1.86e-4, 2.62e-8
    "alpha_20": 918,            # 1.66e-4, 2.65e-8
    "alpha_tiny": 2663,         # 1.46e-4, 2.42e-8
    "all": 142,                 # 2.17e-4, 2.41e-8
}


def twenty_updates(case, seed, device, fused_too=True, updates=20, n=384):
    """The 20 updates of a case on the float64 spec (and, with fused_too, on the fused trainer and the fp32 spec); returns
    ((margin, hidden margin), fused, specs, the last update's statistics per dtype, log_alpha before the last update)."""
    hp = HP_CASES[case]
    mem = memory(seed + 1, M=5, steps=8, device=device)
    mods = hp_modules(case, seed, device)
    fused, sp = trainers(mods, **hp) if fused_too else (None, {F64: specs(mods, **hp)[F64]})
    margin, hidden, last, la = math.inf, math.inf, {}, None
    for i in range(updates):
        idx, eps = batch(mem, n, 1000 * seed + 2 * i)
        if fused_too:
            la = float(fused.log_alpha)
            fused.update(mem, idx, eps)
        for dt, s in sp.items():
            if dt == F64:
                smp = sample(mem, idx, F64)
                m = decision_margin(s, smp[3], eps[:, 0:2], s.target_critic_1, s.target_critic_2)
                with HiddenMargin(s.critic_1, s.critic_2) as hc:
                    st = s.critic_step(*smp, eps[:, 0:2])
                st.pop("y")
                m = min(m, decision_margin(s, smp[0], eps[:, 2:4], s.critic_1, s.critic_2))
                with HiddenMargin(s.policy, s.critic_1, s.critic_2) as hp_:
                    st.update(s.policy_step(smp[0], eps[:, 2:4]))
                s.polyak()
                margin, hidden, last[dt] = min(margin, m), min(hidden, hc.value, hp_.value), st
                if (margin < MARGIN or hidden < HIDDEN_20) and not fused_too:
                    return (margin, hidden), None, sp, last, la                # the seed search stops at the first miss
            else:
                last[dt] = s.update(mem, idx, eps)
    return (margin, hidden), fused, sp, last, la


@pytest.mark.parametrize("case", list(HP_CASES))
def test_twenty_updates_with_moved_hparams_and_the_adam_scalars(case):
    (margin, hidden), fused, sp, last, la = twenty_updates(case, TWENTY_SEEDS[case], DEV)
    print(f"{case}: margin {margin:.3e} hidden {hidden:.3e}")
    assert margin >= MARGIN and hidden >= HIDDEN_20, (margin, hidden)
    check_params(fused, sp)
    check_targets(fused, sp)
    st = fused.stats()
    check_stats(st, last[F64], last[F32], CRITIC_STATS + POLICY_STATS, log_alpha=la)
    assert (st["critic_step"], st["actor_step"], st["entropy_step"], st["bad_index"]) == (20, 20, 20, 0)
    check_adam_scalars(fused, st, (20, 20, 20))


# Unequal clocks: seed 1 has a float64 margin of 2.49e-4 and a hidden margin of 1.37e-7 over the five steps (seed 0: 5e-8)
CLOCK_SEED = 1
CLOCK_HP = dict(actor_lr=1e-3, critic_lr=2e-5, entropy_lr=5e-2, beta1=0.8, beta2=0.99, eps=1e-4)


def unequal_clocks(seed, device, fused_too=True, n=300):
    """critic, critic, policy (with its entropy step), critic, then learn_entropy off and one more policy step: the three Adam
    clocks end at (3, 2, 1).  Returns ((float64 margin, hidden margin), fused, specs)."""
    mem = memory(seed + 1, device=device)
    mods = hp_modules("clocks", seed, device)
    fused, sp = trainers(mods, **CLOCK_HP) if fused_too else (None, {F64: specs(mods, **CLOCK_HP)[F64]})
    margin, hidden = math.inf, math.inf
    for i, step in enumerate(("critic", "critic", "policy", "critic", "policy_without_entropy")):
        idx, eps = batch(mem, n, 100 * seed + 2 * i)
        if step == "policy_without_entropy":
            if fused_too:
                fused.hp.learn_entropy = 0
            for s in sp.values():
                s.hp["learn_entropy"] = False
        for dt, s in sp.items():
            smp = sample(mem, idx, dt)
            if step == "critic":
                if dt == F64:
                    margin = min(margin, decision_margin(s, smp[3], eps[:, 0:2], s.target_critic_1, s.target_critic_2))
                with HiddenMargin(s.critic_1, s.critic_2) as h:
                    s.critic_step(*smp, eps[:, 0:2])
            else:
                if dt == F64:
                    margin = min(margin, decision_margin(s, smp[0], eps[:, 2:4], s.critic_1, s.critic_2))
                with HiddenMargin(s.policy, s.critic_1, s.critic_2) as h:
                    s.policy_step(smp[0], eps[:, 2:4])
            if dt == F64:
                hidden = min(hidden, h.value)
        if fused_too:
            (fused.critic_step if step == "critic" else fused.policy_step)(mem, idx, eps)
    return (margin, hidden), fused, sp


def test_the_three_adam_clocks_run_apart():
    """With critic_step == actor_step == entropy_step, as after any number of whole updates, a final kernel that hands one
    optimiser another's scalars is invisible in the scalars' bias corrections; here the clocks stand at 3, 2 and 1."""
    (margin, hidden), fused, sp = unequal_clocks(CLOCK_SEED, DEV)
    print(f"clocks: margin {margin:.3e} hidden {hidden:.3e}")
    assert margin >= MARGIN and hidden >= HIDDEN, (margin, hidden)
    st = fused.stats()
    assert (st["critic_step"], st["actor_step"], st["entropy_step"], st["bad_index"]) == (3, 2, 1, 0)
    s64 = sp[F64]
    clocks = [opt.state[opt.param_groups[0]["params"][0]]["step"]
              for opt in (s64.critic_optimizer, s64.policy_optimizer, s64.entropy_optimizer)]
    assert [int(t) for t in clocks] == [3, 2, 1]
    check_params(fused, sp)
    check_adam_scalars(fused, st, (3, 2, 1))


# ---------------------------------------------------------------------------------------------------------------- B
# Sampling is with replacement, so a memory of 1200 rows serves every n.  Seeds per n (networks seed, memory seed + 1, batch
# seed + 2), the first from 0 on that meets the single steps' conditions: seed 0 up to n = 511, with margins of 5.4e-3 (n = 1),
# 2.4e-2 (15, 16, 17), 3.3e-3 (63, 65), 1.7e-3 (255, 257), 6.2e-4 (511) and a hidden margin of 1.56e-7 from n = 15 on (the batches
# of one seed share their first rows); seed 13 at n = 513 (4.8e-4, 4.0e-7); seed 34 at n = 1025 (2.5e-4, 2.0e-7)
ROW_SEEDS = {1: 0, 15: 0, 16: 0, 17: 0, 63: 0, 65: 0, 255: 0, 257: 0, 511: 0, 513: 13, 1025: 34}


def row_setup(seed, device=DEV, fused_too=True):
    mem = memory(seed + 1, M=4, N=300, steps=5, device=device)
    mods = hp_modules("rows", seed, device)
    fused, sp = trainers(mods) if fused_too else (None, {F64: specs(mods)[F64]})
    return mem, fused, sp


@pytest.mark.parametrize("n", list(ROW_SEEDS))
def test_row_counts_with_statistics(n):
    seed = ROW_SEEDS[n]
    mem, fused, sp = row_setup(seed)
    idx, eps = batch(mem, n, seed + 2)
    margin, got, _, _ = full_step(mem, fused, sp, idx, eps)
    print(f"n={n}: margin {margin:.3e} hidden {got['hidden']:.3e}")
    assert margin >= MARGIN and got["hidden"] >= HIDDEN, (margin, got["hidden"])


def test_65537_rows_take_the_strided_reduction():
    """65537 rows are 257 reduction blocks: the first count at which reduce_rows' thread 0 adds a second partial, with SAC's five
    and four terms.  The workspace is about 1.9 GB.  Among that many rows some row sits on a clamp or min decision closer than
    the precisions agree, so only what is continuous in those decisions is compared: y, both critics' gradients and the eight
    statistics -- not u, logp, dL/dmu, the actor's gradient or the parameters after Adam."""
    from isaac_rover_orbit_amd import _lib
    n = 65537
    mem, fused, sp = row_setup(72)           # seeds 70 and 71 leave q1_mean at 2e-4 and -2e-3: too close to 0 for the rule
    idx, eps = batch(mem, n, 74)
    full_step(mem, fused, sp, idx, eps, continuous_only=True)
    assert fused.ws.numel() == _lib.load().rover_sac_workspace_bytes(n) > 1.8e9


# ---------------------------------------------------------------------------------------------------------------- C
def stepped(fused, mem, idx, eps, poison_rows=0):
    """critic step, policy step, Polyak; with poison_rows the workspace is regrown and NaN-filled before each step."""
    n = idx.numel()
    out = [torch.empty(n, device=DEV), torch.empty(n, 2, device=DEV), torch.empty(n, device=DEV), torch.empty(n, 2, device=DEV)]
    if poison_rows:
        poison_ws(fused, poison_rows)
    fused.critic_step(mem, idx, eps, y_out=out[0])
    if poison_rows:
        poison_ws(fused, poison_rows)
    fused.policy_step(mem, idx, eps, u_out=out[1], logp_out=out[2], dmean_out=out[3])
    fused.polyak()
    return out


def pair(seed, **mem_kw):
    mem = memory(seed + 1, **mem_kw)
    mods = hp_modules("workspace", seed)
    return mem, trainers(mods)[0], trainers(mods)[0]


@pytest.mark.parametrize("n", [1, 17, 300, 513])
def test_oversized_workspace_full_of_nans_changes_nothing(n):
    from isaac_rover_orbit_amd import _lib
    mem, fresh, dirty = pair(31)
    assert_same_trainer(fresh, dirty)
    idx, eps = batch(mem, n, 100 + n)
    big = 2048
    a, b = stepped(fresh, mem, idx, eps), stepped(dirty, mem, idx, eps, poison_rows=big)
    need = _lib.load().rover_sac_workspace_bytes
    assert fresh.ws.numel() == need(n) and dirty.ws.numel() == need(big) > need(n)
    assert all(bool(torch.isfinite(x).all()) for x in a) and bool(torch.isfinite(fresh.params).all())
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert_same_trainer(fresh, dirty)


@pytest.mark.parametrize("large,small", [(1000, 17), (1100, 513), (600, 1)])
def test_small_step_after_large_step_reads_only_what_it_wrote(large, small):
    mem, one, two = pair(32, N=128)
    stepped(one, mem, *batch(mem, large, 33))
    clone_trainer(one, two)                      # the same starting state, but a workspace that never saw the large step
    idx, eps = batch(mem, small, 35)
    a, b = stepped(one, mem, idx, eps), stepped(two, mem, idx, eps)
    assert one.ws.numel() > two.ws.numel()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert_same_trainer(one, two)
    st = one.stats()
    assert (st["critic_step"], st["actor_step"], st["entropy_step"]) == (2, 2, 2) and bool(torch.isfinite(one.params).all())
