"""The lift rollout collector's specification (isaac_rover_orbit_amd.lift_rollout.TorchLiftRollout) and the error behaviour of its
C ABI (include/rover_lift_rollout.h), on a host without a GPU.

  * with the noise injected, ``act`` reproduces the per-step glue of examples/05_train_lift.py bit for bit (LiftMLP networks, a
    RunningStandardScaler with statistics away from the initial ones on states and values)
  * the draws are ``standard_normals(..., tag=0x4C524F00)``: a stream apart from the rover collector's and from the lift env's
  * two shards of 8 + 9 envs equal one 17-env call bit for bit; the checkpoint resumes the stream
  * ``record`` matches the example's reward / done / episode-tally lines over log vectors with k = 0, 1 and 3
  * rover_lift_rollout_act / rover_lift_rollout_record return codes for bad arguments, nothing is launched
  * the case lists of tests/test_gpu_lift_rollout_edges.py (tests/lift_rollout_helpers.py) on the spec: every action width, the moved
    log-std window, NaN rows under ``clip_actions=True`` (NaN kept), ids that wrap past 2**31 and 2**32, the record kernel's inputs
"""
import ctypes as C

import numpy as np
import pytest
import torch

from isaac_rover_orbit_amd import lift_ppo as LP
from isaac_rover_orbit_amd import lift_rollout as LR
from isaac_rover_orbit_amd import rollout as R
import lift_rollout_helpers as H
from lift_rollout_helpers import TAG, _biteq


@pytest.fixture(scope="module")
def setup():
    """LiftMLP actor / critic, a per-column log_std inside, above and below the clamps, and both scalers trained on two batches."""
    torch.manual_seed(3)
    policy, value = LP.LiftMLP(LP.ACT_DIM, log_std=True), LP.LiftMLP(1)
    with torch.no_grad():
        policy.log_std_parameter.copy_(torch.tensor([0.0, -0.7, 0.3, 2.5, -21.0, 1.0, -3.0, 0.1]))
    sp, vp = LP.RunningStandardScaler(LP.OBS_DIM, device="cpu"), LP.RunningStandardScaler(1, device="cpu")
    g = torch.Generator().manual_seed(4)
    for _ in range(2):
        sp(torch.randn(64, LP.OBS_DIM, generator=g) * 3.0 + 1.5, train=True)
        vp(torch.randn(64, 1, generator=g) * 2.0 - 1.5, train=True)
    assert not torch.equal(sp.running_mean, torch.zeros(LP.OBS_DIM, dtype=torch.float64)) and float(vp.running_variance) != 1.0
    return policy, value, sp, vp


def _spec(setup, n, T=3, rowwise=False, **kw):
    policy, value, sp, vp = setup
    if rowwise:   # one row per call: torch's CPU GEMM picks its blocking (and so its summation order) by the batch size
        net_p, net_v = policy, value
        policy = lambda x: torch.cat([net_p(x[i:i + 1]) for i in range(x.shape[0])])      # noqa: E731
        value = lambda x: torch.cat([net_v(x[i:i + 1]) for i in range(x.shape[0])])       # noqa: E731
    return LR.TorchLiftRollout(policy, value, setup[0].log_std_parameter, lambda x: sp(x), lambda v: vp(v, inverse=True), n, T, **kw)


def _rows(n, seed=0):
    return torch.randn(n, LP.OBS_DIM, generator=torch.Generator().manual_seed(seed)) * 4.0 + 1.0     # some land beyond the scaler's +-5


def test_act_reproduces_the_example_with_injected_noise(setup):
    policy, value, sp, vp = setup
    n = 33
    o = _rows(n)
    eps = torch.randn(n, LP.ACT_DIM, generator=torch.Generator().manual_seed(9))
    # examples/05_train_lift.py, the body of the rollout loop up to env.step (clip_actions: False)
    with torch.no_grad():
        log_std = policy.log_std_parameter.detach()
        std = log_std.clamp(-20.0, 2.0).exp()
        s = sp(o)
        mean = policy(s)
        a = mean + std * eps
        logp = LP.gaussian_logp(mean, log_std, a)
        val = vp(value(s), inverse=True).squeeze(1)
    assert (s.abs() == 5.0).any()                                                         # the scaler's clamp fires
    col = _spec(setup, n)
    env_act = col.act(1, o, eps=eps)
    assert _biteq(env_act, a) and _biteq(col.actions[1], a) and _biteq(col.mean[1], mean)
    assert _biteq(col.logp[1], logp) and _biteq(col.val[1], val) and _biteq(col.obs[1], o)   # the RAW rows are stored
    assert (col.obs[0] == 0).all() and (col.logp[2] == 0).all() and col.counter == 1
    assert _biteq(col.last_value({"policy": o}), val) and col.counter == 1               # the bootstrap value: no draw
    raw = LR.TorchLiftRollout(policy, value, policy.log_std_parameter, lambda x: sp(x), None, n, 1)
    raw.act(0, o, eps=eps)
    with torch.no_grad():
        assert _biteq(raw.val[0], value(s).squeeze(1))                                   # no value scaler: the raw critic output
    clip = _spec(setup, n, clip_actions=True)
    assert _biteq(clip.act(0, o, eps=eps), a.clamp(-1.0, 1.0)) and _biteq(clip.actions[0], a) and (a.abs() > 1.0).any()
    with pytest.raises(ValueError):
        col.act(0, o[:5])
    with pytest.raises(ValueError):
        col.act(0, o.double())


def test_draws_come_from_a_stream_of_their_own(setup):
    n = 17
    col = _spec(setup, n, seed=(7 << 32) | 5, env_id_offset=100)
    ids = 100 + np.arange(n)
    for k in (0, 1, 2 ** 32 + 3):
        col.counter = k
        want = R.standard_normals((7 << 32) | 5, ids, k, LP.ACT_DIM, tag=TAG)
        assert np.array_equal(col.draws(), want) and want.shape == (n, LP.ACT_DIM) and np.isfinite(want).all()
        assert (want != R.standard_normals((7 << 32) | 5, ids, k, LP.ACT_DIM)).all()      # the rover collector's tag
        assert np.array_equal(R.standard_normals((7 << 32) | 5, ids, k, LP.ACT_DIM), R.standard_normals((7 << 32) | 5, ids, k, LP.ACT_DIM, tag=R.ROLLOUT_TAG))
    assert LR.LIFT_ROLLOUT_TAG == TAG != R.ROLLOUT_TAG
    # word 3 of the Philox input: the tag | pair, never 0 or a small 1 + k (the lift env's reset / command draws)
    c3 = np.asarray(R.rollout_counter(ids.reshape(-1, 1), 5, np.arange(4).reshape(1, -1), TAG)[3])
    assert set(int(x) for x in c3.ravel()) == {TAG | p for p in range(4)}
    col.counter = 0
    o = _rows(n)
    col.act(0, o)
    with torch.no_grad():
        policy, _, sp, _ = setup
        mean = policy(sp(o))
        std = policy.log_std_parameter.detach().clamp(-20.0, 2.0).exp()
        eps = torch.from_numpy(R.standard_normals((7 << 32) | 5, ids, 0, LP.ACT_DIM, tag=TAG).astype(np.float32))
    assert _biteq(col.actions[0], mean + std * eps)


def test_shards_equal_the_whole(setup):
    o = _rows(17, seed=2)
    whole = _spec(setup, 17, seed=11, rowwise=True)
    lo, hi = _spec(setup, 8, seed=11, env_id_offset=0, rowwise=True), _spec(setup, 9, seed=11, env_id_offset=8, rowwise=True)
    for t in range(2):
        ea = whole.act(t, o)
        assert _biteq(ea, torch.cat([lo.act(t, o[:8]), hi.act(t, o[8:])]))
    for name in ("obs", "actions", "mean", "logp", "val"):
        w = getattr(whole, name)
        assert _biteq(w, torch.cat([getattr(lo, name), getattr(hi, name)], dim=1)), name
    assert not torch.equal(whole.actions[0], whole.actions[1])                            # the counter moved the draws


def test_checkpoint_resumes_the_stream(setup):
    o = _rows(9, seed=5)
    a = _spec(setup, 9, seed=(3 << 32) | 1, env_id_offset=40)
    a.act(0, o); a.act(1, o)
    sd = a.state_dict()
    assert sd == {"seed": (3 << 32) | 1, "counter": 2, "env_id_offset": 40}
    b = _spec(setup, 9)
    b.load_state_dict(sd)
    assert b.state_dict() == sd
    assert _biteq(a.act(2, o), b.act(2, o)) and _biteq(a.logp[2], b.logp[2]) and a.counter == b.counter == 3
    c = _spec(setup, 9)                                                                   # a fresh stream differs
    assert not torch.equal(c.act(2, o), a.actions[2])


def test_record_matches_the_example_tally(setup):
    n, T = 21, 3
    col = _spec(setup, n, T)
    hp_scale = float(np.float32(0.01))
    g = torch.Generator().manual_seed(6)
    ep_sum, ep_count = torch.zeros(8), torch.zeros(())
    rew_buf, done_buf = torch.zeros(T, n), torch.zeros(T, n)
    for t, k in enumerate((0.0, 1.0, 3.0)):
        rew = torch.randn(n, generator=g)
        term, trunc = torch.rand(n, generator=g) < 0.3, torch.rand(n, generator=g) < 0.3
        log = torch.randn(16, generator=g)
        log[8] = k
        # examples/05_train_lift.py, after env.step
        rew_buf[t] = rew * hp_scale
        done_buf[t] = (term | trunc).float()
        kk = log[8]
        ep_sum += torch.where(kk > 0, log[0:8] * torch.where(torch.arange(8) < 6, kk, 1.0), 0.0)
        ep_count += kk
        col.record(t, rew, term.to(torch.uint8) if t == 1 else term, trunc, log)
        if t == 0:
            assert (col.ep_sum == 0).all() and float(col.ep_count) == 0.0                 # k = 0: nothing is added
    assert _biteq(col.rew, rew_buf) and _biteq(col.done, done_buf) and _biteq(col.ep_sum, ep_sum)
    assert float(col.ep_count) == float(ep_count) == 4.0 and (col.ep_sum != 0).all()
    before = col.ep_sum.clone()
    col.record(0, torch.ones(n), torch.zeros(n, dtype=torch.bool), torch.ones(n, dtype=torch.bool))    # no log: no tally
    assert torch.equal(col.ep_sum, before) and (col.done[0] == 1).all() and _biteq(col.rew[0], torch.ones(n) * hp_scale)
    col.reset_tally()
    assert (col.ep_sum == 0).all() and float(col.ep_count) == 0.0


def test_abi_defaults_and_error_codes():
    """Return codes, not crashes, and nothing launched: every call here fails its argument checks."""
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    hp = LR.default_hparams()
    assert (hp.seed_lo, hp.seed_hi, hp.env_id_offset, hp.clip_actions) == (42, 0, 0, 0)
    assert (hp.action_low, hp.action_high, hp.log_std_min, hp.log_std_max) == (-1.0, 1.0, -20.0, 2.0)
    assert hp.scaler_eps == np.float32(1e-8) and hp.scaler_clip == 5.0 and hp.reward_scale == np.float32(0.01)
    assert lib.rover_lift_rollout_hparams_bytes() == C.sizeof(_lib.LiftRolloutHparams) == 44
    assert lib.rover_lift_rollout_default_hparams(None) == 1
    lift_a, lift_c, rover = _lib.PolicyDesc(), _lib.PolicyDesc(), _lib.PolicyDesc()
    assert lib.rover_lift_policy_desc(C.byref(lift_a), 8) == 0 and lib.rover_lift_policy_desc(C.byref(lift_c), 1) == 0
    assert lib.rover_policy_default_desc(C.byref(rover), 2, 2) == 0
    buf = np.zeros(4096, np.float64)                                                       # host memory: never dereferenced
    p = buf.ctypes.data
    assert p % 16 == 0

    def act(a=lift_a, c=lift_c, h=hp, n=4, obs=p, obs_out=p + 1024, packed=p, sc=p, n_copies=1):
        return lib.rover_lift_rollout_act(C.byref(a), packed, C.byref(c), packed, n_copies, C.byref(h) if h is not None else None,
                                          C.c_uint64(0), obs, n, p, sc, None, obs_out, p, p, None, None, None, None, None)
    assert act(a=rover, c=rover) == 4 and b"rover_lift_policy_desc" in lib.rover_last_error()      # ROVER_ERR_UNSUPPORTED
    assert act(c=lift_a) == 4 and act(a=lift_c, c=lift_a) == 4                             # the critic must have one output
    wide = _lib.PolicyDesc()
    assert lib.rover_lift_policy_desc(C.byref(wide), 17) == 0 and act(a=wide) == 4          # more than one column tile
    assert act(n=0) == 1 and act(n_copies=0) == 1 and act(obs=None) == 1 and act(h=None) == 1 and act(sc=None) == 1
    assert act(obs_out=p) == 1 and b"alias" in lib.rover_last_error()
    assert act(packed=p + 4) == 1 and act(sc=p + 4) == 1                                    # alignment
    bad = LR.default_hparams(); bad.log_std_min = 3.0
    assert act(h=bad) == 1
    bad = LR.default_hparams(); bad.clip_actions, bad.action_low = 1, 2.0
    assert act(h=bad) == 1
    rec = lib.rover_lift_rollout_record
    assert rec(None, p, p, 4, C.c_float(0.01), None, p, p, None, None, None) == 1
    assert rec(p, p, p, 0, C.c_float(0.01), None, p, p, None, None, None) == 1
    assert rec(p, p, p, 4, C.c_float(0.01), p, p, p, None, p, None) == 1                   # a log vector needs ep_sum and ep_count
    if not torch.cuda.is_available():
        with pytest.raises(_lib.RoverHipError):
            LR.LiftRolloutCollector(None, 4, 2)                                            # no CPU fallback


# ------------------------------------------------- the edge cases of tests/test_gpu_lift_rollout_edges.py, on the specification
def _width_spec(A, n, **kw):
    """TorchLiftRollout on the fp32 torch networks of ``width_state_dicts(A)`` and a RunningStandardScaler holding the hand-written
    blocks of ``scaler_blocks``."""
    sd_p, sd_v = H.width_state_dicts(A)
    policy, value = LP.LiftMLP(A), LP.LiftMLP(1)
    policy.load_state_dict(sd_p); value.load_state_dict(sd_v)
    state, vblk = H.scaler_blocks()
    sp, vp = LP.RunningStandardScaler(LP.OBS_DIM, device="cpu"), LP.RunningStandardScaler(1, device="cpu")
    sp.running_mean, sp.running_variance = torch.from_numpy(state[:36]), torch.from_numpy(state[36:72])
    vp.running_mean, vp.running_variance = torch.from_numpy(vblk[:1]), torch.from_numpy(vblk[1:2])
    col = LR.TorchLiftRollout(policy, value, torch.from_numpy(H.log_std_of(A)), lambda x: sp(x), lambda v: vp(v, inverse=True), n, 1, **kw)
    return col, (sd_p, sd_v, torch.from_numpy(state), torch.from_numpy(vblk))


def _outputs(col, t=0):
    eps = (col.actions[t] - col.mean[t]).double()      # not the draws: the measures take eps from the caller
    return {"mean": col.mean[t], "act": col.actions[t], "logp": col.logp[t], "eps": eps}


@pytest.mark.parametrize("A", H.WIDTHS)
def test_action_widths_on_the_spec(A):
    """Every width of the GPU file: shapes, the three sampling bounds on the spec's own fp32 arithmetic, the odd last column as the
    cosine draw of its pair, nesting of the draws, and mean / val within the float64 bound on inputs that respect its cap."""
    worst = 0.0
    for n in H.WIDTH_ROWS:
        o = H.lift_rows(n, seed=n)
        col, (sd_p, sd_v, state, vblk) = _width_spec(A, n, seed=9, env_id_offset=11)
        col.counter = 5
        eps64 = col.draws()
        col.act(0, o)
        assert col.mean[0].shape == col.actions[0].shape == (n, A) and col.logp[0].shape == (n,)
        ls = np.clip(H.log_std_of(A).astype(np.float64), -20.0, 2.0)
        assert (H.log_std_of(A) > 2.0).any() and (A == 1 or (H.log_std_of(A) < -20.0).any())
        out = {"mean": col.mean[0], "act": col.actions[0], "logp": col.logp[0], "eps": torch.from_numpy(eps64.astype(np.float32))}
        H.check_sampling(out, n, ls, f"spec A={A} n={n}", counter=5, seed=9, offset=11)
        wide = R.standard_normals(9, 11 + np.arange(n), 5, A + 1, tag=TAG)
        assert np.array_equal(wide[:, :A], eps64)                                          # column c depends on c, not on A
        if A % 2:
            pair = R.standard_normals(9, 11 + np.arange(n), 5, 2, tag=TAG | ((A - 1) // 2))[:, 0]
            assert np.array_equal(eps64[:, A - 1], pair)                                   # the cosine draw of pair (A - 1) / 2
        ref = H.float64_forward(sd_p, sd_v, o, state, vblk, 1e-8, 5.0)
        worst = max(worst, float(ref[2].double().mean()))
        assert not ref[3].any()
        if n == 33:
            H.check_float64({"mean": col.mean[0], "val": col.val[0].reshape(n, 1)}, ref, f"spec A={A} n={n}")
            assert 0.2 <= float(ref[0].abs().mean()) <= 5.0                                # the means are O(1)
    assert worst <= H.MAX_EXCLUDED


@pytest.mark.parametrize("window", H.WINDOWS)
def test_moved_log_std_window_on_the_spec(window):
    A, n = 8, 33
    ls_raw = torch.tensor(H.LOG_STD)
    col = LR.TorchLiftRollout(lambda s: s[:, :A] * 0.5, lambda s: s[:, :1], ls_raw, lambda x: x, None, n, 1, log_std_min=window[0],
                              log_std_max=window[1])
    eps64 = col.draws()
    col.act(0, H.lift_rows(n, seed=1))
    ls = np.clip(np.array(H.LOG_STD, dtype=np.float32).astype(np.float64), *window)
    out = {"mean": col.mean[0], "act": col.actions[0], "logp": col.logp[0], "eps": torch.from_numpy(eps64.astype(np.float32))}
    H.check_sampling(out, n, ls, f"spec window {window}")
    base = LR.TorchLiftRollout(lambda s: s[:, :A] * 0.5, lambda s: s[:, :1], ls_raw, lambda x: x, None, n, 1)
    base.act(0, H.lift_rows(n, seed=1))
    assert not torch.equal(base.actions[0], col.actions[0]) and _biteq(base.mean[0], col.mean[0])
    assert _biteq(base.logp[0], LP.gaussian_logp(base.mean[0], ls_raw, base.actions[0]))   # the default window is gaussian_logp


@pytest.mark.parametrize("n", H.POISON_ROWS)
def test_nan_rows_stay_nan_under_clip_actions(setup, n):
    """torch.clamp keeps a NaN: the env action of a poisoned row is NaN, not -1; rows with infinities only stay finite."""
    policy, value, sp, vp = setup
    rowwise = lambda net: (lambda x: torch.cat([net(x[i:i + 1]) for i in range(x.shape[0])]))      # noqa: E731
    make = lambda: LR.TorchLiftRollout(rowwise(policy), rowwise(value), policy.log_std_parameter, lambda x: sp(x),      # noqa: E731
                                       lambda v: vp(v, inverse=True), n, 1, seed=7, env_id_offset=3, clip_actions=True)
    o = H.lift_rows(n, seed=2)
    raw, nan_rows, inf_rows = H.poison(o)
    a, b = make(), make()
    eps64 = a.draws()
    env_act, env_clean = a.act(0, raw), b.act(0, o)
    f32 = lambda x: torch.from_numpy(x.astype(np.float32))      # noqa: E731
    out = {"obs": a.obs[0], "mean": a.mean[0], "val": a.val[0], "act": a.actions[0], "env_act": env_act, "logp": a.logp[0], "eps": f32(eps64)}
    clean = {"obs": b.obs[0], "mean": b.mean[0], "val": b.val[0], "act": b.actions[0], "env_act": env_clean, "logp": b.logp[0], "eps": f32(eps64)}
    bad = nan_rows + inf_rows
    clean["obs"] = clean["obs"].clone(); clean["obs"][bad] = raw[bad]
    H.check_poisoned(out, clean, raw, nan_rows, inf_rows, eps64)
    assert ((env_act[inf_rows] >= -1.0) & (env_act[inf_rows] <= 1.0)).all()
    with torch.no_grad():
        assert _biteq(sp(raw)[inf_rows].abs().max(1).values, torch.full((len(inf_rows),), 5.0))      # +-inf standardises to +-clip


def test_ids_wrap_mod_2_32():
    """standard_normals takes ids mod 2**32 (the kernel's word 0 is a uint32 sum): ids past 2**31 and past 2**32, negative ids, the
    by-hand evaluation at the top of every range, and two shards across 2**31 equal to the whole."""
    from td3_helpers import eps_float64_by_hand
    n, A = 33, 3
    for off in H.WRAP_OFFSETS:
        ids = off + np.arange(n, dtype=np.int64)
        assert ids[0] < 2 ** 31 <= ids[-1]
        for counter in H.TOP_COUNTERS:
            got = R.standard_normals(H.TOP_SEED, ids, counter, A, tag=TAG)
            assert np.abs(got - np.array(eps_float64_by_hand(H.TOP_SEED, ids, counter, A, TAG))).max() <= 1e-12
            assert np.array_equal(got, R.standard_normals(H.TOP_SEED, ids + 2 ** 32, counter, A, tag=TAG))
            assert np.array_equal(got, R.standard_normals(H.TOP_SEED, ids - 2 ** 32, counter, A, tag=TAG))
            assert np.array_equal(got, R.standard_normals(H.TOP_SEED, ids.astype(np.uint32).astype(np.int32), counter, A, tag=TAG))
            col = LR.TorchLiftRollout(lambda s: s[:, :A] * 0.5, lambda s: s[:, :1], torch.zeros(A), lambda x: x, None, n, 1, seed=H.TOP_SEED,
                                      env_id_offset=off)
            col.counter = counter
            assert np.array_equal(col.draws(), got)
            lo = LR.TorchLiftRollout(col.actor, col.critic, torch.zeros(A), lambda x: x, None, 16, 1, seed=H.TOP_SEED, env_id_offset=off)
            hi = LR.TorchLiftRollout(col.actor, col.critic, torch.zeros(A), lambda x: x, None, 17, 1, seed=H.TOP_SEED, env_id_offset=off + 16)
            lo.counter = hi.counter = counter
            o = H.lift_rows(n, seed=3)
            whole = col.act(0, o)
            assert _biteq(whole, torch.cat([lo.act(0, o[:16]), hi.act(0, o[16:])])) and _biteq(col.logp[0], torch.cat([lo.logp[0], hi.logp[0]]))


@pytest.mark.parametrize("n", H.RECORD_NS)
def test_record_edge_inputs_on_the_spec(n):
    for seed, scale in enumerate(H.RECORD_SCALES + (1.0,)):
        rew, term, trunc = H.record_inputs(n, seed)
        want_r, want_d = H.expected_record(rew, term, trunc, scale)
        for flags in ((term, trunc), (term != 0, trunc != 0)):
            col = LR.TorchLiftRollout(None, None, torch.zeros(8), None, None, n, 1, reward_scale=scale)
            col.record(0, rew, flags[0], flags[1])
            assert H.same_bits_nan_aware(col.rew[0], want_r) and _biteq(col.done[0], want_d), (scale, flags[0].dtype)
        assert set(term.tolist()) <= set(H.FLAG_VALUES) and (n < 255 or set(term.tolist()) == set(H.FLAG_VALUES))
        assert torch.isnan(rew).any() or n == 1
    col = LR.TorchLiftRollout(None, None, torch.zeros(8), None, None, n, 1)
    col.record(0, rew, term, trunc, H.record_log(2.0, 1))
    for k in H.STILL_KS:
        s0, c0 = col.ep_sum.clone(), col.ep_count.clone()
        assert (s0 != 0).all() and float(c0) == 2.0
        col.record(0, rew, term, trunc, H.record_log(k, 2))
        assert _biteq(col.ep_sum, s0) and _biteq(col.ep_count, c0), k                      # nothing moves, not even a sign of zero
    log = H.record_log(3.0, 3, nan_at=2)
    want_s, want_c = H.expected_tally(col.ep_sum, col.ep_count, log)
    col.record(0, rew, term, trunc, log)
    assert torch.isnan(col.ep_sum[2]) and torch.isfinite(col.ep_sum[[0, 1, 3, 4, 5, 6, 7]]).all() and float(col.ep_count) == 5.0
    assert H.same_bits_nan_aware(col.ep_sum, want_s) and _biteq(col.ep_count, want_c)
