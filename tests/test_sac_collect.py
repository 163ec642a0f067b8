"""The SAC collector's specification (isaac_rover_orbit_amd.sac_collect: TorchSACCollector, cephes_expf, head, random_actions) and the
error behaviour of its C ABI (include/rover_sac_collect.h), on a host without a GPU.

  * driven over two wraps of the ring, the spec leaves a memory bit-equal to nan_to_num + ReplayMemory.add with the same actions
  * cephes_expf against float64 exp; head against sac.gaussian_act in float64; a NaN in mu or log_std stays a NaN
  * the draws do not depend on how the envs are split, and the checkpoint is the counter
  * RANDOM below random_timesteps, then SAMPLE; MEAN draws nothing and still advances the counter
  * the two new tags and every earlier tag have pairwise distinct upper 24 bits
  * the struct mirror and its defaults; every refusal of the header returns its code, nothing is launched
  * the example's parser knows --rollout, and main refuses the fused rollout on the torch update
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from isaac_rover_orbit_amd import rollout as R
from isaac_rover_orbit_amd import sac_collect as SC
from isaac_rover_orbit_amd import td3_collect as TC
from isaac_rover_orbit_amd import td3_explore as TX
from isaac_rover_orbit_amd.sac import gaussian_act
from isaac_rover_orbit_amd.td3 import ReplayMemory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
LOG_STDS = [(0.5, -1.0), (2.5, -25.0), (2.0, -20.0)]
# cephes_expf over 20 000 uniform values in [-20, 2] lies within 1.27 * 2**-24 relative of float64 exp (measured on the CPU, printed by
# test_cephes_expf); the bound on sigma is three times that
SIGMA_TOL = 2.0 ** -22


def _biteq(a, b):
    if a.dtype == torch.bool or b.dtype == torch.bool:
        return a.dtype == b.dtype and torch.equal(a, b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _rows(n, step, seed=0):
    """(n, 965) rows with -inf (ray misses), NaN, +inf and -0.0 at places that move with the step."""
    g = torch.Generator().manual_seed(1000 * seed + step)
    raw = torch.randn(n, 965, generator=g)
    raw[torch.rand(n, 965, generator=g) < 1.0 / 16.0] = float("-inf")
    raw[step % n, 5 + step] = float("nan")
    raw[(step + 1) % n, 964] = float("inf")
    raw[0, 0] = -0.0
    return raw


def _actor(o):
    """A stand-in tanh actor: elementwise in the rows, so a shard's rows are the whole's."""
    return torch.tanh(torch.stack([o[:, 4:100].sum(1) * 0.03, o[:, 0] - o[:, 200:260].sum(1) * 0.05], 1))


def _transition(n, step):
    g = torch.Generator().manual_seed(77 + step)
    rew = torch.randn(n, generator=g)
    rew[step % n] = float("nan") if step % 2 else float("-inf")
    return rew, torch.rand(n, generator=g) < 0.4


def _col(n, M, log_std=(0.5, -1.0), **kw):
    return SC.TorchSACCollector(_actor, torch.tensor(log_std), ReplayMemory(M, n, device="cpu"), **kw)


# --------------------------------------------------------------------------------------------------------------------- the ring
def test_memory_equals_nan_to_num_and_add():
    n, M, steps, B = 5, 2, 5, 7                                       # the ring (3 slots) wraps twice
    col, ref = _col(n, M, seed=9), ReplayMemory(M, n, device="cpu")
    col.begin(_rows(n, 0))
    o = torch.nan_to_num(_rows(n, 0), neginf=0.0)
    for t in range(steps):                                            # the torch loop of examples/09_train_sac.py
        a = col.act(t).clone()
        assert _biteq(a, col.memory.actions[col.memory.memory_index]) and float(a.abs().max()) <= 1.0
        rew, term = _transition(n, t)
        counter = col.counter
        idx, eps = col.record(_rows(n, t + 1), rew, term, B)
        o_next = torch.nan_to_num(_rows(n, t + 1), neginf=0.0)
        ref.add(o, a, rew, o_next, term)
        o = o_next
        assert idx.dtype == torch.int64 and idx.shape == (B,) and int(idx.min()) >= 0 and int(idx.max()) < min(t + 1, M) * n
        assert idx.tolist() == TC.sample_indices(9, counter, B, len(col.memory)).tolist()
        assert eps.dtype == torch.float32 and eps.shape == (B, 4)
        assert np.array_equal(eps.numpy(), TX.smooth_normals(9, counter, B, 4).astype(F))
        assert col.counter == 2 * (t + 1)
    mem = col.memory
    assert not torch.isfinite(_rows(n, 1)).all() and torch.isfinite(mem.obs).all()
    for name in ("obs", "actions", "rewards", "terminated", "ring_pos"):
        assert _biteq(getattr(mem, name), getattr(ref, name)), name
    assert len(mem) == len(ref) == M * n and (mem.memory_index, mem.filled, mem.cursor) == (ref.memory_index, ref.filled, ref.cursor)
    assert mem.filled and bool((mem.obs.view(torch.int32) == -(1 << 31)).any())             # -0.0 passes as it is
    rew, term = _transition(n, 9)
    assert col.record(_rows(n, 9), rew, term) is None and col.counter == 2 * steps + 1


# --------------------------------------------------------------------------------------------------------------------- the head
def test_cephes_expf():
    x = np.random.RandomState(0).uniform(-20.0, 2.0, 20000).astype(F)
    got = SC.cephes_expf(x)
    rel = np.abs(got.astype(np.float64) / np.exp(x.astype(np.float64)) - 1.0).max()
    print(f"cephes_expf: max relative error over 20000 values in [-20, 2] = {rel / 2.0 ** -24:.3f} * 2**-24")
    assert got.dtype == F and rel <= 1.27 * 2.0 ** -24
    edge = SC.cephes_expf(np.array([np.nan, 0.0, -0.0, 89.0, -89.0, np.inf, -np.inf], F))
    assert np.isnan(edge[0]) and edge[1:].tolist() == [1.0, 1.0, np.inf, 0.0, np.inf, 0.0]
    assert np.isnan(SC.cephes_expf(F(np.nan)))
    assert SC.cephes_expf(F(2.0)) == F(7.389056) and SC.cephes_expf(F(-20.0)) == F(2.0611537e-09)


def _head_inputs(log_std, n=257):
    """mu and eps of a case.  A column whose clamped log_std is -20 has sigma = 2.06e-9, under half an ulp of any |mu| >= 2**-6: there
    fp32 rounds x = mu + sigma * eps back to mu and t = (u - mu) / sigma is 0 for ANY fp32 evaluation in the kernel's order (the fused
    update's head included), where float64 keeps t = eps; no bound in units of float32 roundings relates the two (with tanh means in
    that column too, the same 257 rows give max |dlogp| = 4.69 at log_std (2.5, -25) and (2, -20), 37 678 times 1e-5 |logp| + 1e-5,
    while u and sigma stay within their bounds).  In such a column the means are multiples of 2**-30 up to 8 sigma, the range in
    which fp32 carries both mu and the draw, so the comparison with float64 checks the formula; every other column takes tanh means
    over (-1, 1)."""
    rng = np.random.RandomState(5)
    mu = np.tanh(rng.standard_normal((n, 2)) * 1.2).astype(F)
    eps = rng.standard_normal((n, 2)).astype(F)
    for c in range(2):
        if log_std[c] <= -20.0:
            mu[:, c] = (rng.randint(-16, 17, n) * 2.0 ** -30).astype(F)
    return mu, eps


@pytest.mark.parametrize("log_std", LOG_STDS)
def test_head_against_gaussian_act_in_float64(log_std):
    mu, eps = _head_inputs(log_std)
    u, logp, sigma = SC.head(mu, log_std, eps)
    assert u.dtype == logp.dtype == sigma.dtype == F and u.shape == (257, 2) and logp.shape == (257,) and sigma.shape == (2,)
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))   # noqa: E731
    u64, logp64 = gaussian_act(t64(mu), t64(log_std), t64(eps))
    d_u = np.abs(u.astype(np.float64) - u64.numpy()).max()
    d_lp = np.abs(logp.astype(np.float64) - logp64.numpy()[:, 0])
    s64 = np.exp(np.clip(np.asarray(log_std, dtype=np.float64), -20.0, 2.0))
    d_s = np.abs(sigma.astype(np.float64) / s64 - 1.0).max()
    print(f"log_std {log_std}: max |du| {d_u:.3e}, max |dlogp| / (1e-5 |logp| + 1e-5) {(d_lp / (1e-5 * np.abs(logp64.numpy()[:, 0]) + 1e-5)).max():.3e}, "
          f"sigma {d_s / 2.0 ** -24:.3f} * 2**-24; {int((np.abs(u) == 1).sum())} of {u.size} clamped")
    assert d_u <= 1e-6
    assert (d_lp <= 1e-5 * np.abs(logp64.numpy()[:, 0]) + 1e-5).all()
    assert d_s <= SIGMA_TOL
    assert (np.abs(u) == 1).any() and (np.abs(u) < 1).any() and np.abs(u).max() <= 1.0
    if log_std == (0.5, -1.0):                                          # the clamp is exercised at both bounds
        assert (u == 1).any() and (u == -1).any()
    if log_std[1] == -25.0:                                             # outside the clamp: the result is the bound's
        assert np.array_equal(sigma, SC.head(mu, (2.0, -20.0), eps)[2]) and np.array_equal(u, SC.head(mu, (2.0, -20.0), eps)[0])


def test_nan_stays_nan():
    mu, eps = _head_inputs((0.5, -1.0), n=9)
    mu[3, 0] = np.nan
    u, logp, sigma = SC.head(mu, (0.5, -1.0), eps)
    assert np.isnan(u[3, 0]) and np.isnan(logp[3]) and np.isfinite(np.delete(u.reshape(-1), 6)).all() and np.isfinite(sigma).all()
    u, logp, sigma = SC.head(np.nan_to_num(mu), (np.nan, -1.0), eps)     # a NaN log_std: its column is NaN, the other is not touched
    assert np.isnan(u[:, 0]).all() and np.isnan(sigma[0]) and np.isfinite(u[:, 1]).all() and sigma[1] == SC.cephes_expf(F(-1.0))
    assert np.array_equal(u[:, 1], SC.head(np.nan_to_num(mu), (0.5, -1.0), eps)[0][:, 1])
    assert np.isnan(SC.tclamp(F(np.nan), -1.0, 1.0)) and SC.tclamp(np.array([-np.inf, np.inf, -0.5], F), -1.0, 1.0).tolist() == [-1.0, 1.0, -0.5]
    # through the collector: a NaN mean reaches the memory as NaN, not as -1
    col = SC.TorchSACCollector(lambda o: torch.full((4, 2), float("nan")), torch.tensor([0.5, -1.0]), ReplayMemory(2, 4, device="cpu"))
    col.begin(_rows(4, 0))
    assert torch.isnan(col.act(0)).all() and torch.isnan(col.memory.actions[0]).all()


# -------------------------------------------------------------------------------------------------------------------- the draws
def test_draws_do_not_depend_on_the_split():
    seed, counter = (9 << 32) | 5, (1 << 32) | 7
    whole = SC.action_normals(seed, np.arange(33), counter)
    parts = np.concatenate([SC.action_normals(seed, 0 + np.arange(16), counter), SC.action_normals(seed, 16 + np.arange(17), counter)])
    assert whole.shape == (33, 2) and np.array_equal(whole, parts)
    assert np.array_equal(whole, R.standard_normals(seed, np.arange(33), counter, 2, tag=SC.ACTION_TAG))
    assert not np.array_equal(whole, R.standard_normals(seed, np.arange(33), counter, 2, tag=TC.NOISE_TAG))
    ra = SC.random_actions(seed, np.arange(33), counter)
    assert np.array_equal(ra, np.concatenate([SC.random_actions(seed, np.arange(16), counter), SC.random_actions(seed, 16 + np.arange(17), counter)]))
    # ... and through the collectors: shards of 16 and 17 envs against the 33-env whole
    w = _col(33, 4, seed=seed, random_timesteps=1)
    ps = [_col(m, 4, seed=seed, env_id_offset=off, random_timesteps=1) for m, off in ((16, 0), (17, 16))]
    sl = (slice(0, 16), slice(16, 33))
    raw = _rows(33, 0)
    w.begin(raw)
    for p, s in zip(ps, sl):
        p.begin(raw[s])
    for t in range(3):
        a, b = w.act(t), torch.cat([p.act(t) for p in ps])
        assert _biteq(a, b)
        rew, term = _transition(33, t)
        raw = _rows(33, t + 1)
        w.record(raw, rew, term)
        for p, s in zip(ps, sl):
            p.record(raw[s], rew[s].contiguous(), term[s].contiguous())
    assert _biteq(w.memory.actions, torch.cat([p.memory.actions for p in ps], 1))


def test_random_actions_by_hand():
    seed, counter, ids = (3 << 32) | 42, (1 << 32) | 7, np.array([0, 5, 2 ** 31 - 2])
    w = R.philox4x32(ids.astype(np.uint64), counter & 0xFFFFFFFF, counter >> 32, 0x53415200, seed & 0xFFFFFFFF, seed >> 32)
    got = SC.random_actions(seed, ids, counter)
    for c in range(2):
        u = ((w[c] >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        assert np.array_equal(got[:, c], (F(-1.0) + (F(2.0) * u.astype(F)).astype(F)).astype(F))
    big = SC.random_actions(1, np.arange(4096), 0)
    assert big.dtype == F and big.min() > -1.0 and big.max() < 1.0 and abs(float(big.mean())) < 0.05 and big.std() > 0.5


def test_checkpoint_is_the_counter():
    n, M = 6, 5
    col = _col(n, M, seed=11, env_id_offset=32)
    col.begin(_rows(n, 0))
    acts, batches = [], []
    for t in range(4):
        if t == 2:
            sd = col.state_dict()
            assert sd == {"seed": 11, "counter": 4, "env_id_offset": 32}
            fresh = _col(n, M)
            fresh.load_state_dict(sd)
            for name in ("obs", "actions", "rewards", "terminated", "ring_pos"):
                getattr(fresh.memory, name).copy_(getattr(col.memory, name))
            fresh.memory.cursor, fresh.memory.memory_index, fresh.memory.filled = col.memory.cursor, col.memory.memory_index, col.memory.filled
        acts.append(col.act(t).clone())
        rew, term = _transition(n, t)
        batches.append(col.record(_rows(n, t + 1), rew, term, 33))
    for t in (2, 3):                                                   # the restored collector reproduces steps 3 and 4
        assert _biteq(fresh.act(t), acts[t])
        rew, term = _transition(n, t)
        idx, eps = fresh.record(_rows(n, t + 1), rew, term, 33)
        assert torch.equal(idx, batches[t][0]) and _biteq(eps, batches[t][1])
    assert fresh.state_dict() == col.state_dict() and col.counter == 8
    assert not _biteq(acts[2], acts[3])


def test_modes():
    n = 8
    col = _col(n, 4, seed=3, env_id_offset=10, random_timesteps=2)
    assert [col.mode(t) for t in range(4)] == [SC.RANDOM, SC.RANDOM, SC.SAMPLE, SC.SAMPLE] and col.mode(0, True) == SC.MEAN
    col.begin(_rows(n, 0))
    mean = _actor(col.memory.obs[col.memory.cursor])
    ids = 10 + np.arange(n)
    a0 = col.act(0)
    assert np.array_equal(a0.numpy(), SC.random_actions(3, ids, 0)) and col.last == {} and col.counter == 1
    a1 = col.act(1)
    assert np.array_equal(a1.numpy(), SC.random_actions(3, ids, 1)) and not _biteq(a0, a1)
    a2 = col.act(2)
    eps = SC.action_normals(3, ids, 2).astype(F)
    u, logp, sigma = SC.head(mean.numpy(), (0.5, -1.0), eps)
    assert np.array_equal(a2.numpy(), u) and np.array_equal(col.last["logp"].numpy(), logp) and np.array_equal(col.last["eps"].numpy(), eps)
    assert np.array_equal(col.last["sigma"].numpy(), sigma) and _biteq(col.last["mean"], mean) and col.counter == 3
    given = torch.from_numpy(np.random.RandomState(1).standard_normal((n, 2)).astype(F))
    a3 = col.act(3, eps=given)                                         # a given eps replaces the float64 draw
    assert np.array_equal(a3.numpy(), SC.head(mean.numpy(), (0.5, -1.0), given.numpy())[0]) and col.counter == 4
    a4 = col.act(0, deterministic=True)                                # MEAN, also below random_timesteps: no draw, the counter moves
    assert _biteq(a4, mean) and set(col.last) == {"mean"} and col.counter == 5 and _biteq(col.memory.actions[0], mean)
    # log_std is read at every act: the collector follows the trainer's tensor
    col.log_std.copy_(torch.tensor([-3.0, -3.0]))
    a5 = col.act(5)
    assert np.array_equal(a5.numpy(), SC.head(mean.numpy(), (-3.0, -3.0), SC.action_normals(3, ids, 5).astype(F))[0])
    with pytest.raises(ValueError):
        SC.TorchSACCollector(_actor, torch.zeros(2), ReplayMemory(2, n, device="cpu", act_dim=3))
    with pytest.raises(ValueError):
        col.record(_rows(n, 1), *_transition(n, 0), 0)


def test_tags_have_distinct_upper_24_bits():
    assert SC.TAGS == {"sac_action": 0x53414300, "sac_random": 0x53415200}
    tags = {**TX.TAGS, **SC.TAGS}                                       # the repository's table lists the two as well
    assert len(tags) == 9 and set(SC.TAGS.items()) <= set(TX.TAGS.items())
    upper = [t >> 8 for t in tags.values()]
    assert len(set(upper)) == len(upper) and all(t & 0xFF == 0 for t in tags.values())


# ---------------------------------------------------------------------------------------------------------------------- the ABI
def test_struct_and_defaults():
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    assert lib.rover_sac_collect_hparams_bytes() == C.sizeof(_lib.SacCollectHparams) == 16
    assert lib.rover_sac_collect_default_hparams(None) == 1
    hp = SC.default_hparams()
    assert (hp.seed_lo, hp.seed_hi, hp.env_id_offset, hp.mode) == (42, 0, 0, SC.SAMPLE)
    assert (SC.SAMPLE, SC.MEAN, SC.RANDOM) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "rover_sac_collect.h")).read()
    for name, value in (("ROVER_SAC_COLLECT_SAMPLE", "0"), ("ROVER_SAC_COLLECT_MEAN", "1"), ("ROVER_SAC_COLLECT_RANDOM", "2"),
                        ("ROVER_SAC_TAG_ACTION", "0x53414300u"), ("ROVER_SAC_TAG_RANDOM", "0x53415200u")):
        assert f"#define {name} {value}" in " ".join(hdr.split())


def test_abi_errors_are_codes():
    """Every refusal of the header: ROVER_ERR_INVALID (1), or ROVER_ERR_UNSUPPORTED (4) for an actor that is not the reference
    architecture with two tanh outputs.  Nothing reaches the GPU: the checks come before any HIP call."""
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    hp = SC.default_hparams()
    tanh, plain, wide = _lib.PolicyDesc(), _lib.PolicyDesc(), _lib.PolicyDesc()
    assert lib.rover_policy_default_desc(C.byref(tanh), 2, 1) == 0 and lib.rover_policy_default_desc(C.byref(plain), 2, 0) == 0
    assert lib.rover_policy_default_desc(C.byref(wide), 3, 1) == 0
    # never dereferenced: every call below is refused before a launch
    P, LS, OBS, OUT, RING, EPS = 0x10000, 0x18000, 0x20000, 0x30000, 0x4000000, 0x50000
    good = dict(actor=C.byref(tanh), p=P, copies=1, ls=LS, hp=C.byref(hp), counter=0, obs=OBS, n=16, mean=None, act=OUT, env_act=OUT,
                eps=None, logp=None, sigma=None)

    def act(**kw):
        a = dict(good, **kw)
        return lib.rover_sac_collect_act(a["actor"], a["p"], a["copies"], a["ls"], a["hp"], C.c_uint64(a["counter"]), a["obs"], a["n"],
                                         a["mean"], a["act"], a["env_act"], a["eps"], a["logp"], a["sigma"], None)

    assert lib.rover_sac_collect_act(None, None, 0, None, None, C.c_uint64(0), None, 0, None, None, None, None, None, None, None) == 1
    assert len(lib.rover_last_error()) > 0
    for bad in (dict(actor=None), dict(hp=None), dict(p=None), dict(obs=None), dict(act=None), dict(env_act=None), dict(n=0), dict(n=-3),
                dict(copies=0), dict(p=P + 4), dict(ls=None)):
        assert act(**bad) == 1, bad
    for mode in (3, -1, 99):
        bad_hp = _lib.SacCollectHparams.from_buffer_copy(hp)
        bad_hp.mode = mode
        assert act(hp=C.byref(bad_hp)) == 1 and b"mode" in lib.rover_last_error()
    lift = _lib.PolicyDesc()
    assert lib.rover_lift_policy_desc(C.byref(lift), 8) == 0
    for d in (plain, wide, lift):
        assert act(actor=C.byref(d)) == 4 and b"tanh" in lib.rover_last_error()
    for mode in (SC.MEAN, SC.RANDOM):                                   # ... in every mode
        m_hp = _lib.SacCollectHparams.from_buffer_copy(hp)
        m_hp.mode = mode
        assert act(hp=C.byref(m_hp), actor=C.byref(plain)) == 4 and act(hp=C.byref(m_hp), n=0, ls=None) == 1

    rgood = dict(raw=OBS, n=16, ring=RING, rew=OUT, term=OUT, rew_out=OUT, term_out=OUT, pos=OUT, pos_value=0, idx=OUT, batch=8, rows=16,
                 eps=EPS, hp=C.byref(hp))

    def rec(**kw):
        a = dict(rgood, **kw)
        return lib.rover_sac_collect_record(a["raw"], a["n"], a["ring"], a["rew"], a["term"], a["rew_out"], a["term_out"], a["pos"],
                                            a["pos_value"], a["idx"], a["batch"], a["rows"], a["eps"], a["hp"], C.c_uint64(0), None)

    assert lib.rover_sac_collect_record(None, 1, None, None, None, None, None, None, 0, None, 0, 0, None, None, C.c_uint64(0), None) == 1
    for bad in (dict(raw=None), dict(ring=None), dict(n=0), dict(n=-1), dict(ring=OBS), dict(ring=OBS + 4), dict(ring=OBS + 16 * 965 * 4 - 4),
                dict(raw=RING + 4), dict(rows=0), dict(rows=-5), dict(rows=2 ** 32 + 1), dict(batch=0), dict(hp=None), dict(rew=None),
                dict(term=None), dict(rew_out=None), dict(term_out=None), dict(rew=None, rew_out=None), dict(eps=EPS + 4), dict(eps=EPS + 8),
                dict(idx=None, eps=EPS + 12), dict(idx=None, batch=0), dict(idx=None, hp=None)):
        assert rec(**bad) == 1, bad
    assert rec(ring=OBS) == 1 and b"alias" in lib.rover_last_error()
    assert rec(rows=0) == 1 and b"mem_rows" in lib.rover_last_error()
    assert rec(eps=EPS + 4) == 1 and b"aligned" in lib.rover_last_error()
    if not torch.cuda.is_available():
        with pytest.raises(_lib.RoverHipError):
            SC.SACCollector(None, None, ReplayMemory(2, 4, device="cpu"))        # the product path fails loudly, no CPU fallback


# ------------------------------------------------------------------------------------------------------------------ the example
def test_example_parser_knows_the_fused_rollout(capsys):
    spec = importlib.util.spec_from_file_location("train_sac_example", os.path.join(ROOT, "examples", "09_train_sac.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    assert ex.build_parser().parse_args([]).rollout == "torch"
    args = ex.build_parser().parse_args(["--rollout", "fused", "--update", "fused", "--random_timesteps", "5"])
    assert (args.rollout, args.update, args.random_timesteps) == ("fused", "fused", 5)
    with pytest.raises(SystemExit):
        ex.main(["--rollout", "fused", "--update", "torch"])
    assert "--update fused" in capsys.readouterr().err
