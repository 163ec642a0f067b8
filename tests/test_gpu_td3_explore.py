"""TD3's exploration switches on the MI355X (include/rover_td3_explore.h, isaac_rover_orbit_amd.td3_explore) against the collector's
kernel and the specification.  Random packed weights and synthetic rows, n in {1, 15, 16, 17, 33}: one lane, a ragged workgroup, one
workgroup and the edges of two.

  * OFF / GAUSSIAN: mean, act, env_act and eps BIT-EXACT against rover_td3_collect_act
  * OU over three consecutive calls: ou_state and act BIT-EXACT against the spec fed the device's own eps (no transcendental enters);
    its eps is GAUSSIAN's on the bits; a NaN state entry stays where it is; the other modes never touch ou_state
  * RANDOM BIT-EXACT against the spec, independent of the packed weights and of the split over calls; mean / eps untouched
  * rover_td3_smooth_draw against the float64 Box-Muller at EPS_TOL of tests/test_gpu_td3_collect.py, the prefix property, the
    sample moments, and through FusedTD3.update against TorchTD3.update at the tolerance of tests/test_gpu_td3_update.py
  * TD3Explorer against TorchTD3Explorer over the wrap of a four-slot memory: random steps, then OU
"""
import numpy as np
import pytest
import torch

from rollout_helpers import _biteq, synthetic_rows
from td3_helpers import same_bits_nan_aware
from test_gpu_td3_collect import EPS_TOL, SENTINEL, _act, _actor, _step_inputs

pytestmark = pytest.mark.gpu

NS = [1, 15, 16, 17, 33]
OUT_KEYS = ("mean", "act", "env_act", "eps")


@pytest.fixture(scope="module")
def actor():
    return _actor(2)


@pytest.fixture(scope="module")
def clean():
    """(33, 965) sanitised rows, as a ring slot holds them."""
    return torch.nan_to_num(synthetic_rows(33, seed=0), nan=0.0, neginf=0.0).contiguous()


def _xhp(**kw):
    from isaac_rover_orbit_amd import td3_explore as TE
    hp = TE.default_hparams()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def _xact(actor, rows, counter=0, ou_state=None, **hp):
    """One explore launch into sentinel-filled outputs; returns mean, act, env_act, eps."""
    from isaac_rover_orbit_amd import td3_explore as TE
    n, A = rows.shape[0], actor.out_dim
    o = {k: torch.full((n, A), SENTINEL, dtype=torch.float32, device="cuda") for k in OUT_KEYS}
    TE.explore_act(actor, rows, counter, _xhp(**hp), o["act"], o["env_act"], ou_state=ou_state, mean_out=o["mean"], eps_out=o["eps"])
    torch.cuda.synchronize()
    return o


# ---------------------------------------------------------------------------------------------------------- OFF and GAUSSIAN
@pytest.mark.parametrize("n", NS)
def test_off_and_gaussian_are_the_collector_on_the_bits(actor, clean, n):
    from isaac_rover_orbit_amd import td3_explore as TE
    rows = clean[:n].contiguous()
    want_mean = actor(rows)
    for counter in (0, 7, 2 ** 32 + 5):
        for offset in (0, 1000):
            kw = dict(seed_lo=9, seed_hi=5, env_id_offset=offset, noise_std=0.3, noise_scale=0.7, action_low=-0.25, action_high=0.5)
            for mode, explore in ((TE.OFF, 0), (TE.GAUSSIAN, 1)):
                got = _xact(actor, rows, counter, mode=mode, **kw)
                want = _act(actor, rows, counter, explore=explore, **kw)
                for k in OUT_KEYS:
                    assert _biteq(got[k], want[k]), (counter, offset, mode, k)
                assert _biteq(got["mean"], want_mean)
    # OFF does not use the range: reversed bounds are accepted there, as the collector accepts them without exploration
    got = _xact(actor, rows, 3, mode=TE.OFF, action_low=1.0, action_high=-1.0)
    assert _biteq(got["act"], want_mean) and (got["eps"] == SENTINEL).all()
    # mean_out and eps_out are optional
    a, e = torch.full((n, 2), SENTINEL, device="cuda"), torch.full((n, 2), SENTINEL, device="cuda")
    TE.explore_act(actor, rows, 7, _xhp(mode=TE.GAUSSIAN, noise_std=0.5), a, e)
    full = _xact(actor, rows, 7, mode=TE.GAUSSIAN, noise_std=0.5)
    assert _biteq(a, full["act"]) and _biteq(e, full["env_act"])


# ------------------------------------------------------------------------------------------------------------------------ OU
@pytest.mark.parametrize("n", NS)
def test_ou_three_calls_against_the_spec_on_the_device_eps(actor, clean, n):
    from isaac_rover_orbit_amd import td3_explore as TE
    rows = clean[:n].contiguous()
    theta, sigma, base, scale, low, high = 0.15, 0.2, 0.7, 0.9, -0.25, 0.5
    kw = dict(seed_lo=3, seed_hi=1, env_id_offset=200, noise_scale=scale, action_low=low, action_high=high)
    g = torch.Generator(device="cuda").manual_seed(n)
    state = torch.randn(n, 2, device="cuda", generator=g) * 0.3                         # a run under way, not the zero start
    x = state.cpu().numpy().copy()
    hits = 0
    for counter in (2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1):
        o = _xact(actor, rows, counter, ou_state=state, mode=TE.OU, ou_theta=theta, ou_sigma=sigma, ou_base_scale=base, noise_std=123.0, **kw)
        gauss = _xact(actor, rows, counter, mode=TE.GAUSSIAN, noise_std=0.3, **kw)
        assert _biteq(o["eps"], gauss["eps"]) and _biteq(o["mean"], gauss["mean"])      # one noise stream, one forward
        x, noise = TE.ou_step(x, o["eps"].cpu().numpy(), theta, sigma, base)
        want = TE.add_noise_clamp(o["mean"].cpu(), torch.from_numpy(noise), scale, low, high)
        assert _biteq(state.cpu(), torch.from_numpy(x)), counter
        assert _biteq(o["act"].cpu(), want) and _biteq(o["env_act"], o["act"]), counter
        hits += int(((want == low) | (want == high)).sum())
    assert hits > 0 or n == 1                                                           # the clamp was reached
    assert np.abs(x).max() > 0.01


def test_a_nan_state_entry_stays_and_touches_nothing_else(actor, clean):
    from isaac_rover_orbit_amd import td3_explore as TE
    n = 33
    kw = dict(counter=4, mode=TE.OU, noise_scale=0.8)
    g = torch.Generator(device="cuda").manual_seed(1)
    base = torch.randn(n, 2, device="cuda", generator=g) * 0.2
    clean_state, bad_state = base.clone(), base.clone()
    bad_state[16, 1] = float("nan")                                                     # the first row of the second workgroup
    want = _xact(actor, clean, ou_state=clean_state, **kw)
    got = _xact(actor, clean, ou_state=bad_state, **kw)
    assert torch.isnan(bad_state[16, 1]) and torch.isnan(got["act"][16, 1]) and torch.isnan(got["env_act"][16, 1])
    keep = torch.ones(n, 2, dtype=torch.bool, device="cuda")
    keep[16, 1] = False
    assert int(torch.isnan(bad_state).sum()) == 1 and int(torch.isnan(got["act"]).sum()) == 1
    for a, b in ((bad_state, clean_state), (got["act"], want["act"]), (got["env_act"], want["env_act"])):
        assert torch.equal(a[keep].view(torch.int32), b[keep].view(torch.int32))
    assert _biteq(got["eps"], want["eps"]) and _biteq(got["mean"], want["mean"])


@pytest.mark.parametrize("n", [17, 33])
def test_the_other_modes_leave_the_ou_state_alone(actor, clean, n):
    from isaac_rover_orbit_amd import td3_explore as TE
    rows = clean[:n].contiguous()
    buf = torch.full((16 + n * 2 + 16,), SENTINEL, dtype=torch.float32, device="cuda")
    state = buf[16:16 + 2 * n].view(n, 2)
    for mode in (TE.OFF, TE.GAUSSIAN, TE.RANDOM):
        _xact(actor, rows, 5, ou_state=state, mode=mode, noise_std=0.3)
        assert (buf == SENTINEL).all(), mode
    _xact(actor, rows, 5, ou_state=state, mode=TE.OU)                                   # ... and OU writes exactly the (n, 2) values
    assert (state != SENTINEL).all() and (buf[:16] == SENTINEL).all() and (buf[16 + 2 * n:] == SENTINEL).all()


# -------------------------------------------------------------------------------------------------------------------- RANDOM
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("A", [2, 6])
def test_random_is_the_spec_on_the_bits_and_reads_no_actor(clean, n, A):
    from isaac_rover_orbit_amd import td3_explore as TE
    net = _actor(A)
    rows = clean[:n].contiguous()
    seed, offset, low, high = (5 << 32) | 9, 1000, -0.25, 0.75
    kw = dict(mode=TE.RANDOM, seed_lo=9, seed_hi=5, env_id_offset=offset, action_low=low, action_high=high, noise_std=0.3)
    for counter in (0, 7, 2 ** 32 + 5):
        o = _xact(net, rows, counter, **kw)
        want = torch.from_numpy(TE.random_actions(seed, offset + np.arange(n), counter, A, low, high))
        assert _biteq(o["act"].cpu(), want) and _biteq(o["env_act"], o["act"]), counter
        assert (o["mean"] == SENTINEL).all() and (o["eps"] == SENTINEL).all()           # neither is written
        assert bool((o["act"] >= low).all()) and bool((o["act"] <= high).all())
    poisoned = _actor(A)
    poisoned.packed.fill_(float("nan"))
    assert _biteq(_xact(poisoned, rows, 7, **kw)["act"], _xact(net, rows, 7, **kw)["act"])
    assert torch.isnan(_xact(poisoned, rows, 7, **dict(kw, mode=TE.OFF))["act"]).all()  # the poison is real: the actor modes see it


def test_random_split_over_two_calls(actor, clean):
    from isaac_rover_orbit_amd import td3_explore as TE
    kw = dict(counter=4, mode=TE.RANDOM, seed_lo=2)
    whole = _xact(actor, clean[:17].contiguous(), env_id_offset=0, **kw)
    lo = _xact(actor, clean[:9].contiguous(), env_id_offset=0, **kw)
    hi = _xact(actor, clean[9:17].contiguous(), env_id_offset=9, **kw)
    for k in ("act", "env_act"):
        assert _biteq(whole[k], torch.cat([lo[k], hi[k]])), k
    nxt = _xact(actor, clean[:17].contiguous(), env_id_offset=0, **dict(kw, counter=5))
    assert (nxt["act"] != whole["act"]).any()


# -------------------------------------------------------------------------------------------------------- the smoothing draw
def _draw(n, A=2, std=1.0, seed=(5 << 32) | 9, counter=2 ** 32 + 7):
    from isaac_rover_orbit_amd import td3_explore as TE
    buf = torch.full((16 + n * A + 16,), SENTINEL, dtype=torch.float32, device="cuda")
    out = TE.smooth_draw(seed, counter, std, buf[16:16 + n * A].view(n, A))
    torch.cuda.synchronize()
    assert (buf[:16] == SENTINEL).all() and (buf[16 + n * A:] == SENTINEL).all()
    return out


@pytest.fixture(scope="module")
def long_draw():
    return {A: _draw(257, A) for A in (2, 16)}


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
@pytest.mark.parametrize("A", [2, 16])
def test_smooth_draw_against_the_float64_spec_and_its_prefix(long_draw, n, A):
    from isaac_rover_orbit_amd import td3_explore as TE
    one = _draw(n, A)
    ref = TE.smooth_normals((5 << 32) | 9, 2 ** 32 + 7, n, A)
    worst = float(np.abs(one.cpu().numpy().astype(np.float64) - ref).max())
    print(f"n={n} A={A}: max |eps_kernel - eps_float64| = {worst:.3e}; bound {EPS_TOL:.3e}")
    assert worst <= EPS_TOL
    assert _biteq(one, long_draw[A][:n].contiguous())                                   # the prefix of a longer draw
    half = _draw(n, A, std=0.5)
    assert _biteq(half, one * 0.5)                                                      # std * eps: one more fp32 product (exact here)
    assert not _draw(n, A, std=0.0).any()
    assert (_draw(n, A, counter=2 ** 32 + 8) != one).any()


def test_smooth_draw_moments():
    x = _draw(65536, 2, std=0.2, seed=77, counter=3).double()
    mean, std = float(x.mean()), float(x.std())
    print(f"131072 draws at std 0.2: mean {mean:.3e} (bound {5 * 0.2 / np.sqrt(131072):.3e}), std {std:.6f}")
    assert abs(mean) < 5 * 0.2 / np.sqrt(131072)
    assert abs(std - 0.2) < 0.02 * 0.2
    assert abs(float((x[:, 0] * x[:, 1]).mean())) < 5 * 0.04 / np.sqrt(65536)           # the two branches of a pair: uncorrelated


def test_smooth_draw_through_the_update():
    """The draw as the `noise` of FusedTD3.update against TorchTD3.update on the same batch: two updates, so the actor and the targets
    step once; the comparison is check() of tests/td3_helpers.py, as tests/test_gpu_td3_update.py applies it to the smoothed path."""
    from isaac_rover_orbit_amd import td3_explore as TE
    from td3_helpers import check
    from test_gpu_td3_update import DEV, params, setup
    mem, fused, specs = setup(seed=2, bias=(0.8, -0.8))
    n = 512
    g = torch.Generator(device=DEV).manual_seed(8)
    clipped = 0
    for step in range(2):
        idx = mem.sample_indices(n, g)
        noise = TE.smooth_draw(11, step, 0.6, torch.empty(n, 2, device=DEV))            # std above the clip of 0.5: both clamps
        clipped += int((noise.abs() > 0.5).sum())
        stepped = fused.update(mem, idx, noise)
        last = {dt: sp.update(mem, idx, noise) for dt, sp in specs.items()}
        assert all(v["actor_stepped"] == stepped for v in last.values())
    assert clipped > 0 and stepped
    st = fused.stats()
    assert st["critic_step"] == 2 and st["actor_step"] == 1 and st["bad_index"] == 0
    p, t = fused.unvector(fused.params), fused.unvector(fused.target)
    s64, s32 = specs[torch.float64], specs[torch.float32]
    for k, tk in (("policy", "target_policy"), ("critic_1", "target_critic_1"), ("critic_2", "target_critic_2")):
        check(p[k], params(getattr(s64, k)), params(getattr(s32, k)), what=f"{k} ")
        check(t[k], params(getattr(s64, tk)), params(getattr(s32, tk)), what=f"{tk} ")
    assert st["critic_loss"] == pytest.approx(last[torch.float64]["critic_loss"], rel=1e-3)


# ------------------------------------------------------------------------------------------------------------- the explorer
def test_explorer_against_the_spec_over_the_wrap():
    from isaac_rover_orbit_amd import td3_explore as TE
    from isaac_rover_orbit_amd.td3 import FusedTD3, ReplayMemory
    from td3_helpers import nets
    n, M, steps, B, T = 33, 4, 6, 64, 20
    fused = FusedTD3(*(m.state_dict() for m in nets(seed=3)))
    mem, ref = ReplayMemory(M, n, device="cuda"), ReplayMemory(M, n, device="cpu")
    kw = dict(seed=(7 << 32) | 5, env_id_offset=100, noise="ou", clip=(-0.05, 0.05), random_timesteps=2, ou_sigma=0.3)
    col = TE.TD3Explorer(fused.actor, mem, **kw)
    spec = TE.TorchTD3Explorer(lambda o: fused.actor(o.cuda().contiguous()).cpu(), ref, **kw)
    raw0 = _step_inputs(n, 99)[0]
    col.begin(raw0)
    spec.begin({"policy": raw0.cpu()})
    mean = torch.full((n, 2), SENTINEL, device="cuda")
    eps = torch.full((n, 2), SENTINEL, device="cuda")
    for t in range(steps):
        k = mem.memory_index
        a = col.act(t, T, mean_out=mean, eps_out=eps)
        torch.cuda.synchronize()
        if t < 2:
            assert (mean == SENTINEL).all() and (eps == SENTINEL).all() and not col.ou_state.any()
            b = spec.act(t, T)
        else:
            assert np.abs(eps.cpu().numpy() - spec.draws()).max() <= EPS_TOL
            b = spec.act(t, T, eps=eps)                                                 # the device's own draws: bits, not a tolerance
            assert _biteq(mean, fused.actor(mem.obs[mem.cursor])) and (a.abs() == 0.05).any()
        assert _biteq(a.cpu(), b) and _biteq(a, mem.actions[k]) and _biteq(col.ou_state.cpu(), spec.ou_state), t
        raw, rew, term = _step_inputs(n, t)
        i = col.record(raw, rew, term, B)
        j = spec.record(raw.cpu(), rew.cpu(), term.cpu(), B)
        assert torch.equal(i.cpu(), j) and int(i.max()) < len(mem) == min(t + 1, M) * n
        for name in ("obs", "actions", "rewards", "terminated", "ring_pos"):
            x, y = getattr(mem, name).cpu(), getattr(ref, name)
            assert torch.equal(x, y) and (x.dtype != torch.float32 or _biteq(x, y)), (t, name)
        assert (mem.memory_index, mem.filled, mem.cursor) == (ref.memory_index, ref.filled, ref.cursor)
    assert mem.filled and col.counter == spec.counter == 2 * steps
    # the smoothing draw of both, and the checkpoint
    # |eps| < 5.8 (u >= 2**-24), so rounding the spec's float64 eps to fp32 moves 0.2 eps by at most 0.2 x 5.8 x 2**-24 and each side's
    # product is rounded by at most 1.16 x 2**-24: under 3.5 x 2**-24 < 2**-22 together, on top of the draw's own 0.2 x EPS_TOL
    x, y = col.smooth_noise(B, 0.2), spec.smooth_noise(B, 0.2)
    assert (x.cpu() - y).abs().max() <= 0.2 * EPS_TOL + 2.0 ** -22 and col.update_counter == spec.update_counter == 1
    sd = col.state_dict()
    assert sd["counter"] == 12 and sd["update_counter"] == 1 and _biteq(sd["ou_state"], spec.ou_state)
    fused.update(mem, i, x)
    assert fused.stats()["bad_index"] == 0
    other = TE.TD3Explorer(fused.actor, ReplayMemory(M, n, device="cuda"), noise="ou")
    other.load_state_dict(sd)
    assert _biteq(other.ou_state, col.ou_state) and other.counter == 12 and other.seed == (7 << 32) | 5
    assert same_bits_nan_aware(other.smooth_noise(B, 0.2), col.smooth_noise(B, 0.2))
