"""The rollout collector's specification (isaac_rover_orbit_amd.rollout.TorchRollout) and the error behaviour of its C ABI
(include/rover_rollout.h), on a host without a GPU.

  * the spec's Philox4x32-10 (numpy integer arithmetic) equals the oracle's on the Random123 known answers and on random inputs
  * the uniforms are exact in fp32 and strictly inside (0, 1)
  * the Box-Muller draws of seed 42 pass 5-sigma bounds on mean, variance, the correlation inside a pair and the lag-one
    correlation over the counter (the spec is deterministic: these either hold or the transform is wrong)
  * the rollout's Philox inputs are pairwise distinct and disjoint from every env draw's
  * rover_rollout_act / rover_rollout_record return codes for bad arguments, nothing is launched
"""
import ctypes as C

import numpy as np
import pytest
import torch

from isaac_rover_orbit_amd import rollout as R

F = 0xFFFFFFFF


def _philox(*args):
    return [int(x) for x in R.philox4x32(*args)]


def test_spec_philox_matches_the_oracle(oracle):
    kats = [((0, 0, 0, 0, 0, 0), [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
            ((F, F, F, F, F, F), [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0), [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for args, want in kats:
        assert _philox(*args) == want == oracle.philox(*args)
    rng = np.random.RandomState(5)
    x = rng.randint(0, 2 ** 32, size=(1000, 6), dtype=np.uint64)
    got = np.stack(R.philox4x32(*[x[:, i] for i in range(6)]), axis=1)       # the vectorised form, all 1000 at once
    for i in range(1000):
        assert [int(v) for v in got[i]] == oracle.philox(*[int(v) for v in x[i]]), x[i]


def test_uniforms_are_exact_in_fp32_and_inside_the_unit_interval():
    for w in (0, 0x1ff, 0x200, 0xfffffe00, F):
        u = float(R.unit_uniform(w))
        assert 0.0 < u < 1.0
        assert float(np.float32(u)) == u                                       # exact in fp32
        assert u == ((w >> 9) + 0.5) / 2 ** 23
    assert float(R.unit_uniform(0)) == float(R.unit_uniform(0x1ff)) == 2.0 ** -24
    assert float(R.unit_uniform(F)) == 1.0 - 2.0 ** -24


def test_draw_statistics_seed_42():
    """4096 rows x 64 counters x one pair: N = 2**19 draws, 5-sigma bounds of the estimators."""
    n, steps = 4096, 64
    eps = np.stack([R.standard_normals(42, np.arange(n), k, 2) for k in range(steps)])     # (64, 4096, 2) float64
    N = eps.size
    assert N == 2 ** 19 and np.isfinite(eps).all()
    b = 5.0 / np.sqrt(N)
    mean, var = eps.mean(), eps.var()
    corr = np.corrcoef(eps[..., 0].ravel(), eps[..., 1].ravel())[0, 1]
    lag = np.corrcoef(eps[:-1].ravel(), eps[1:].ravel())[0, 1]                               # same row and column, counter k and k + 1
    print(f"mean {mean:.3e} var-1 {var - 1:.3e} corr {corr:.3e} lag {lag:.3e} (bounds {b:.3e}, {5 * np.sqrt(2 / N):.3e})")
    assert abs(mean) <= b
    assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / N)
    assert abs(corr) <= b
    assert abs(lag) <= b
    assert np.abs(eps).max() <= 5.77                                                         # sqrt(-2 ln 2**-24)


def test_odd_width_uses_the_cosine_of_its_last_pair():
    e4, e3 = R.standard_normals(7, np.arange(9), 3, 4), R.standard_normals(7, np.arange(9), 3, 3)
    assert e3.shape == (9, 3) and np.array_equal(e3, e4[:, :3])


def test_stream_separation():
    """64 ids x 8 counters x 8 pairs: no two Philox inputs coincide, and none is an env draw's (word 3 in {0, 1, 2}:
    resets (id, count, block, 0), commands (id, count, 0, 1), the per-step word (counter lo, counter hi, 0x5eed, 2))."""
    seen = set()
    for g in range(64):
        for k in list(range(6)) + [2 ** 32, 2 ** 40 + 1]:
            for p in range(8):
                c = tuple(int(v) for v in R.rollout_counter(g, k, p))
                assert c == (g, k & F, k >> 32, 0x524F4C00 | p)
                assert c not in seen
                seen.add(c)
                assert c[3] not in (0, 1, 2) and (c[3] >> 8) == 0x524F4C
    assert len(seen) == 64 * 8 * 8


def test_torch_rollout_runs_on_the_cpu():
    """The spec end to end with stand-in networks: sanitised rows, the counter, the checkpoint, clip and log-prob."""
    n, T = 33, 3
    g = torch.Generator().manual_seed(0)
    Wa, Wc = torch.randn(965, 2, generator=g) * 0.01, torch.randn(965, 1, generator=g) * 0.01
    actor, critic = (lambda o: torch.tanh(o.clamp(-10, 10) @ Wa)), (lambda o: o.clamp(-10, 10) @ Wc)
    log_std = torch.tensor([0.3, -25.0])                         # the second one sits at the lower clamp
    ro = R.TorchRollout(actor, critic, log_std, n, T, seed=42, env_id_offset=100)
    raw = torch.randn(n, 965, generator=g)
    raw[0, 3], raw[5, 964], raw[7, 10], raw[32, 963] = float("-inf"), float("-inf"), float("nan"), float("inf")
    ea = ro.act(0, raw)
    assert ro.counter == 1 and ea.shape == (n, 2) and float(ea.abs().max()) <= 1.0
    assert torch.equal(ro.obs[0], torch.nan_to_num(raw, nan=0.0, posinf=R.FLT_MAX, neginf=0.0)) and torch.isfinite(ro.obs[0]).all()
    eps = R.standard_normals(42, 100 + np.arange(n), 0, 2)
    std = np.exp(np.array([0.3, -20.0]))
    assert np.allclose(ro.actions[0].numpy(), ro.mean[0].numpy() + std * eps, atol=1e-6)
    # the log-probability is a function of the STORED action (at std = 2e-9 the noise mostly rounds away: x is not eps there)
    x = (ro.actions[0].numpy().astype(np.float64) - ro.mean[0].numpy()) / np.exp(np.array([0.3, -20.0])).astype(np.float32)
    want = (-0.5 * x ** 2 - np.array([0.3, -20.0]) - 0.9189385332).sum(1)
    assert np.allclose(ro.logp[0].numpy(), want, rtol=1e-5, atol=1e-5)
    assert torch.equal(ea, ro.actions[0].clamp(-1, 1))
    ro.record(0, torch.arange(n, dtype=torch.float32), torch.arange(n) % 2 == 0, torch.arange(n) % 3 == 0)
    assert torch.equal(ro.done[0], ((torch.arange(n) % 2 == 0) | (torch.arange(n) % 3 == 0)).float())
    v = ro.last_value(raw)
    assert ro.counter == 1 and v.shape == (n,)
    # a fresh collector resumed from the checkpoint draws what the original draws next; a shard draws its rows of the whole
    ro2 = R.TorchRollout(actor, critic, log_std, n, T, seed=1)
    ro2.load_state_dict(ro.state_dict())
    assert ro2.state_dict() == {"seed": 42, "counter": 1, "env_id_offset": 100}
    assert torch.equal(ro.act(1, raw), ro2.act(1, raw)) and torch.equal(ro.logp[1], ro2.logp[1])
    shard = R.TorchRollout(actor, critic, log_std, 10, T, seed=42, env_id_offset=120)
    shard.counter = 1
    shard.act(1, raw[20:30])
    assert torch.equal(shard.actions[1], ro.actions[1, 20:30])


def test_abi_errors_are_codes():
    """rover_rollout_act(NULL, ...) and every other invalid argument return ROVER_ERR_INVALID (1); a network that is not the
    reference architecture returns ROVER_ERR_UNSUPPORTED (4).  Nothing reaches the GPU: the checks come before any HIP call."""
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    assert lib.rover_rollout_hparams_bytes() == C.sizeof(_lib.RolloutHparams) == 32
    assert lib.rover_rollout_default_hparams(None) == 1
    hp = _lib.RolloutHparams()
    assert lib.rover_rollout_default_hparams(C.byref(hp)) == 0
    assert (hp.seed_lo, hp.seed_hi, hp.env_id_offset, hp.clip_actions) == (42, 0, 0, 1)
    assert (hp.action_low, hp.action_high, hp.log_std_min, hp.log_std_max) == (-1.0, 1.0, -20.0, 2.0)
    da, dc = _lib.PolicyDesc(), _lib.PolicyDesc()
    assert lib.rover_policy_default_desc(C.byref(da), 2, 1) == 0 and lib.rover_policy_default_desc(C.byref(dc), 1, 0) == 0
    # never dereferenced: every call below is refused before a launch
    P, OBS, OUT, LS = 0x10000, 0x20000, 0x30000, 0x40000
    good = dict(actor=C.byref(da), pa=P, critic=C.byref(dc), pb=P, copies=1, hp=C.byref(hp), counter=0, obs=OBS, n=16, ls=LS,
                obs_out=None, mean=OUT, val=OUT, act=None, env_act=None, logp=None, eps=None, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.rover_rollout_act(a["actor"], a["pa"], a["critic"], a["pb"], a["copies"], a["hp"], C.c_uint64(a["counter"]), a["obs"],
                                     a["n"], a["ls"], a["obs_out"], a["mean"], a["val"], a["act"], a["env_act"], a["logp"], a["eps"],
                                     a["stream"])

    assert lib.rover_rollout_act(None, None, None, None, 0, None, C.c_uint64(0), None, 0, None, None, None, None, None, None, None,
                                 None, None) == 1
    assert len(lib.rover_last_error()) > 0
    for bad in (dict(actor=None), dict(critic=None), dict(hp=None), dict(pa=None), dict(pb=None), dict(obs=None), dict(ls=None),
                dict(mean=None), dict(val=None), dict(n=0), dict(n=-3), dict(copies=0), dict(pa=P + 4), dict(pb=P + 8),
                dict(obs_out=OBS)):
        assert call(**bad) == 1, bad
    bad_hp = _lib.RolloutHparams.from_buffer_copy(hp)
    bad_hp.log_std_min, bad_hp.log_std_max = 2.0, -20.0
    assert call(hp=C.byref(bad_hp)) == 1 and b"log_std" in lib.rover_last_error()
    lift = _lib.PolicyDesc()
    assert lib.rover_lift_policy_desc(C.byref(lift), 8) == 0
    assert call(actor=C.byref(lift)) == 4 and call(critic=C.byref(lift)) == 4
    wide = _lib.PolicyDesc.from_buffer_copy(da)
    wide.layers[5].N = 17
    assert call(actor=C.byref(wide)) == 4
    slope = _lib.PolicyDesc.from_buffer_copy(dc)
    slope.leaky_slope = 0.2
    assert call(critic=C.byref(slope)) == 4
    assert lib.rover_rollout_record(None, None, None, 1, None, None, None) == 1
    assert lib.rover_rollout_record(OBS, OBS, OBS, 0, OUT, OUT, None) == 1
    if not torch.cuda.is_available():
        with pytest.raises(_lib.RoverHipError):
            R.RolloutCollector(None, None, torch.zeros(2), 16, 4)               # the product path fails loudly, no CPU fallback
