"""The lift rollout collector's specification (isaac_rover_orbit_amd.lift_rollout.TorchLiftRollout) and the error behaviour of its
C ABI (include/rover_lift_rollout.h), on a host without a GPU.

  * with the noise injected, ``act`` reproduces the per-step glue of examples/05_train_lift.py bit for bit (LiftMLP networks, a
    RunningStandardScaler with statistics away from the initial ones on states and values)
  * the draws are ``standard_normals(..., tag=0x4C524F00)``: a stream apart from the rover collector's and from the lift env's
  * two shards of 8 + 9 envs equal one 17-env call bit for bit; the checkpoint resumes the stream
  * ``record`` matches the example's reward / done / episode-tally lines over log vectors with k = 0, 1 and 3
  * rover_lift_rollout_act / rover_lift_rollout_record return codes for bad arguments, nothing is launched
"""
import ctypes as C

import numpy as np
import pytest
import torch

from isaac_rover_orbit_amd import lift_ppo as LP
from isaac_rover_orbit_amd import lift_rollout as LR
from isaac_rover_orbit_amd import rollout as R

TAG = 0x4C524F00


def _biteq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


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
    # word 3 of the Philox input: the tag | pair, never 0 or 1 (the lift env's reset / command draws)
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
