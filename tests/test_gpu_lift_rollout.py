"""The fused lift rollout step on the MI355X (include/rover_lift_rollout.h, isaac_rover_orbit_amd.lift_rollout) against its
specification.  Synthetic rows, a FusedLiftPPO with random parameters, scaler blocks written by hand: one state column with
variance 0 (the ``+ eps`` path), means of +-3, rows that land beyond +-5 on both sides (both scaler clamps fire), a value scaler
with variance 4 and mean -1.5.

  * obs_out, mean_out, val_out: BIT-EXACT against the input rows, ``trainer.actor(trainer.standardize(o))`` and
    ``trainer.standardize(trainer.critic(s), "value", inverse=True)`` (the raw critic output without a value scaler)
  * eps against the float64 Box-Muller spec: 2.05e-06; act against mean + exp(ls) * eps in float64: 4 ulp of
    max(|mean|, |std * eps|); logp against the float64 formula on the returned act / mean: (8 + (A - 2) / 2) * 2**-23 *
    sum_c (0.5 x_c**2 + |ls_c| + 0.919) -- the bounds DESIGN 16 records for the same operation sequence (A = 8: 11 * 2**-23);
    each figure is printed before it is asserted (DESIGN 17 is where the measured maxima are recorded)
  * counters, shards, live parameters, the bootstrap form, guards around every output, the record kernel and its tally, the
    refusal of the rover's descriptors, and a KL of exactly 0 when FusedLiftPPO.minibatch re-evaluates the collector's own rows
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lift_rollout_helpers import EPS_TOL, FILL, GUARD, LS_CLAMPED, ULP, _biteq, _errors, _make_trainer, _run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 8
LOGP_TOL = (8 + (A - 2) / 2) * ULP


@pytest.fixture(scope="module")
def trainer():
    return _make_trainer()


def _rows(n, seed=0):
    """(n, 36) rows on the GPU: N(1, 4**2), so standardised values pass +5 and -5."""
    o = torch.randn(n, 36, generator=torch.Generator().manual_seed(seed)) * 4.0 + 1.0
    return o.cuda()


def _reference(tr, o):
    s = tr.standardize(o)
    v = tr.critic(s)
    return s, tr.actor(s), v, tr.standardize(v, "value", inverse=True)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, 257])
def test_forward_is_bit_identical_to_the_trainer(trainer, n):
    o = _rows(n)
    o[::3, 7] = float(trainer.state_scaler[7])                    # the variance-0 column at its mean: 0 / 1e-8
    s, mean, v_raw, val = _reference(trainer, o)
    if n >= 15:
        assert (s == 5.0).any() and (s == -5.0).any() and (s[::3, 7] == 0.0).all() and (s[1::3, 7].abs() == 5.0).all()
    out = _run(trainer, o, counter=3, env_id_offset=5)
    assert _biteq(out["obs"], o)                                  # the RAW rows
    assert _biteq(out["mean"], mean) and _biteq(out["val"], val) and torch.isfinite(mean).all() and torch.isfinite(val).all()
    assert not torch.equal(val, v_raw)
    raw = _run(trainer, o, counter=3, env_id_offset=5, value_scaler=False)
    assert _biteq(raw["val"], v_raw) and _biteq(raw["mean"], mean)
    for k in ("act", "env_act", "logp", "eps"):                   # the value scaler touches nothing else
        assert _biteq(raw[k], out[k]), k


def test_draws_and_sampling_within_the_recorded_bounds(trainer):
    worst = [0.0, 0.0, 0.0]
    for n, counter, seed_lo, seed_hi, offset in ((257, 0, 42, 0, 0), (33, 7, 9, 5, 1000), (1, 2, 42, 0, 0)):
        o = _rows(n, seed=n)
        out = _run(trainer, o, counter=counter, seed_lo=seed_lo, seed_hi=seed_hi, env_id_offset=offset)
        d = _errors(out, n, counter, (seed_hi << 32) | seed_lo, offset)
        print(f"n={n}: |eps - spec| {d[0]:.3e}; act {d[1] / ULP:.2f} ulp; logp {d[2] / ULP:.2f} x 2**-23 of the scale")
        worst = [max(a, b) for a, b in zip(worst, d)]
        assert _biteq(out["env_act"], out["act"])                 # clip_actions: False is the default
        clipped = _run(trainer, o, counter=counter, seed_lo=seed_lo, seed_hi=seed_hi, env_id_offset=offset, clip_actions=1)
        assert _biteq(clipped["env_act"], out["act"].clamp(-1.0, 1.0)) and _biteq(clipped["act"], out["act"])
        assert _biteq(clipped["logp"], out["logp"])
        narrow = _run(trainer, o, counter=counter, seed_lo=seed_lo, seed_hi=seed_hi, env_id_offset=offset, clip_actions=1,
                      action_low=-0.25, action_high=0.5)
        assert _biteq(narrow["env_act"], out["act"].clamp(-0.25, 0.5))
        if n > 1:
            assert (out["act"].abs() > 1.0).any()
    print(f"maxima: |eps - spec| {worst[0]:.3e} (bound {EPS_TOL:.3e}); act {worst[1] / ULP:.2f} ulp (4); "
          f"logp {worst[2] / ULP:.2f} x 2**-23 ({LOGP_TOL / ULP:.0f})")
    assert worst[0] <= EPS_TOL
    assert worst[1] <= 4 * ULP
    assert worst[2] <= LOGP_TOL


@pytest.mark.parametrize("counter", [0, 2 ** 32 - 1, 2 ** 32])
def test_counter_words(trainer, counter):
    n = 33
    o = _rows(n, seed=4)
    a, b = _run(trainer, o, counter=counter), _run(trainer, o, counter=counter)
    for k in a:
        assert _biteq(a[k], b[k]), k
    d = _errors(a, n, counter)
    assert d[0] <= EPS_TOL and d[1] <= 4 * ULP and d[2] <= LOGP_TOL
    other = _run(trainer, o, counter=counter + 1)
    assert (a["eps"] != other["eps"]).all()
    for k in ("obs", "mean", "val"):
        assert _biteq(a[k], other[k]), k


def test_two_shards_equal_the_whole(trainer):
    o = _rows(33, seed=6)
    whole = _run(trainer, o, counter=5, env_id_offset=64)
    lo = _run(trainer, o[:17].contiguous(), counter=5, env_id_offset=64)
    hi = _run(trainer, o[17:].contiguous(), counter=5, env_id_offset=64 + 17)
    for k in whole:
        assert _biteq(whole[k], torch.cat([lo[k], hi[k]])), k


def test_null_optional_outputs_and_the_bootstrap_form(trainer):
    from isaac_rover_orbit_amd import lift_rollout as LR
    n = 17
    o = _rows(n, seed=8)
    full = _run(trainer, o, counter=2)
    for outs in (("obs",), ("act",), ("env_act",), ("logp",), ("eps",), ("act", "logp"), ("obs", "env_act", "eps"), ()):
        part = _run(trainer, o, counter=2, outs=outs)
        assert set(part) == set(outs) | {"mean", "val"}
        for k in part:
            assert _biteq(part[k], full[k]), (outs, k)
    col = LR.LiftRolloutCollector(trainer, n, 2, seed=7)
    for buf in (col.obs, col.actions, col.mean, col.logp, col.val, col._env_act):
        buf.fill_(FILL)
    v = col.last_value(o)
    torch.cuda.synchronize()
    assert col.counter == 0 and _biteq(v, _reference(trainer, o)[3][:, 0])
    for buf in (col.obs, col.actions, col.mean, col.logp, col.val, col._env_act):
        assert (buf == FILL).all()                                # no draw, no slot written


def test_collector_slots_checkpoint_and_validation(trainer):
    from isaac_rover_orbit_amd import lift_rollout as LR
    n, T = 17, 3
    o = _rows(n, seed=9)
    col = LR.LiftRolloutCollector(trainer, n, T, seed=(5 << 32) | 9, env_id_offset=64)
    ea0 = col.act(0, o).clone()
    ea1 = col.act(1, {"policy": o}).clone()
    assert col.counter == 2 and not torch.equal(ea0, ea1)
    ref = _run(trainer, o, counter=1, seed_lo=9, seed_hi=5, env_id_offset=64)
    for k, buf in (("obs", col.obs), ("mean", col.mean), ("act", col.actions), ("logp", col.logp)):
        assert _biteq(buf[1], ref[k]), k
    assert _biteq(col.val[1], ref["val"][:, 0]) and _biteq(ea1, ref["act"])       # not clipped
    assert (col.obs[2] == 0).all() and (col.logp[2] == 0).all()                   # slot 2 untouched
    fresh = LR.LiftRolloutCollector(trainer, n, T)
    fresh.load_state_dict(col.state_dict())
    assert fresh.state_dict() == {"seed": (5 << 32) | 9, "counter": 2, "env_id_offset": 64}
    assert _biteq(col.act(2, o), fresh.act(2, o)) and _biteq(col.logp[2], fresh.logp[2])
    # ... and the CPU specification on the kernel's mean / value agrees within the eps bound (same seed, ids and counter)
    spec = LR.TorchLiftRollout(lambda s: col.mean[2].cpu(), lambda s: col.val[2].cpu(), trainer.log_std.cpu(), lambda x: x, None, n, T)
    spec.load_state_dict({"seed": (5 << 32) | 9, "counter": 2, "env_id_offset": 64})
    spec.act(2, o.cpu())
    std_max = float(np.exp(LS_CLAMPED).max())
    assert (spec.actions[2] - col.actions[2].cpu()).abs().max() <= std_max * 2 * EPS_TOL
    with pytest.raises(ValueError):
        col.act(0, o[:5])
    with pytest.raises(ValueError):
        col.act(0, o.cpu())
    with pytest.raises(ValueError):
        col.record(0, torch.zeros(n, device="cuda").double(), torch.zeros(n, dtype=torch.bool, device="cuda"),
                   torch.zeros(n, dtype=torch.bool, device="cuda"))


def test_live_parameters_and_scalers():
    """After one update on a tiny batch the collector's next mean follows the new parameters and the new state scaler: nothing is
    re-packed or re-bound."""
    from isaac_rover_orbit_amd import lift_rollout as LR
    tr = _make_trainer(seed=5, kl_early_stop=0.0)             # the scaler moves under the first minibatch: no early stop
    n, T = 24, 2
    col = LR.LiftRolloutCollector(tr, n, T)
    o = _rows(n, seed=10)
    for t in range(T):
        col.act(t, o if t == 0 else _rows(n, seed=11))
    before, p0, sc0 = col.mean[0].clone(), tr.params.clone(), tr.state_scaler.clone()
    g = torch.Generator(device="cuda").manual_seed(1)
    adv, ret = torch.randn(T, n, device="cuda", generator=g), torch.randn(T, n, device="cuda", generator=g)
    val_s = tr.standardize(col.val.reshape(-1, 1).contiguous(), "value", train=True).reshape(T, n)
    tr.update(col.obs, col.actions, col.logp, val_s, ret, adv, epochs=1, minibatches=2)
    assert not torch.equal(tr.params, p0) and not torch.equal(tr.state_scaler, sc0) and tr.steps >= 1
    col.act(0, o)
    _, mean, _, val = _reference(tr, o)
    assert _biteq(col.mean[0], mean) and _biteq(col.val[0], val[:, 0]) and not torch.equal(col.mean[0], before)
    ls = tr.log_std.clamp(-20.0, 2.0)
    x = (col.actions[0] - mean) / ls.exp()
    assert torch.allclose(col.logp[0], (-0.5 * x * x - ls - 0.9189385332).sum(1), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_record_and_the_episode_tally(n):
    from isaac_rover_orbit_amd import lift_rollout as LR
    g = torch.Generator().manual_seed(n)
    for scale, as_bool in ((0.01, True), (1.0, False)):
        spec = LR.TorchLiftRollout(None, None, torch.zeros(A), None, None, n, 3, reward_scale=scale)
        rew_out, done_out = (torch.full((3, n + 2 * GUARD), FILL, device="cuda") for _ in range(2))
        ep = torch.full((8 + 2 * GUARD,), FILL, device="cuda")
        ep_sum = ep[GUARD:GUARD + 8]
        ep_sum.zero_()
        ep_count = torch.zeros((), device="cuda")
        for t, k in enumerate((0.0, 1.0, 3.0)):
            rew = torch.randn(n, generator=g)
            term, trunc = torch.rand(n, generator=g) < 0.3, torch.rand(n, generator=g) < 0.3
            log = torch.randn(16, generator=g)
            log[8] = k
            spec.record(t, rew, term, trunc, log)
            flags = [f.cuda() if as_bool else f.to(torch.uint8).cuda() for f in (term, trunc)]
            LR.lift_rollout_record(rew.cuda(), flags[0], flags[1], float(np.float32(scale)), rew_out[t, GUARD:GUARD + n],
                                   done_out[t, GUARD:GUARD + n], log.cuda(), ep_sum, ep_count)
            if t == 0:
                torch.cuda.synchronize()
                assert (ep_sum == 0).all() and float(ep_count) == 0.0                 # k = 0 adds nothing
        torch.cuda.synchronize()
        assert _biteq(rew_out[:, GUARD:GUARD + n].cpu(), spec.rew) and _biteq(done_out[:, GUARD:GUARD + n].cpu(), spec.done)
        assert _biteq(ep_sum.cpu(), spec.ep_sum) and float(ep_count) == float(spec.ep_count) == 4.0
        for buf in (rew_out, done_out):
            assert (buf[:, :GUARD] == FILL).all() and (buf[:, GUARD + n:] == FILL).all()
        assert (ep[:GUARD] == FILL).all() and (ep[GUARD + 8:] == FILL).all()
        if scale == 1.0:
            assert _biteq(rew_out[2, GUARD:GUARD + n].cpu(), rew)
        # log = NULL: no tally (ep_sum / ep_count are not even passed)
        before = ep_sum.clone()
        LR.lift_rollout_record(rew.cuda(), flags[0], flags[1], 1.0, rew_out[0, GUARD:GUARD + n], done_out[0, GUARD:GUARD + n])
        torch.cuda.synchronize()
        assert torch.equal(ep_sum, before) and float(ep_count) == 4.0 and _biteq(rew_out[0, GUARD:GUARD + n].cpu(), rew)


def test_collector_record_uses_the_trainers_reward_scale(trainer):
    from isaac_rover_orbit_amd import lift_rollout as LR
    n = 33
    col = LR.LiftRolloutCollector(trainer, n, 2)
    g = torch.Generator(device="cuda").manual_seed(2)
    rew = torch.randn(n, device="cuda", generator=g)
    term, trunc = torch.rand(n, device="cuda", generator=g) < 0.3, torch.rand(n, device="cuda", generator=g) < 0.3
    log = torch.rand(16, device="cuda", generator=g)
    log[8] = 2.0
    col.record(1, rew, term, trunc, log)
    assert _biteq(col.rew[1], rew * trainer.hp.reward_scale) and _biteq(col.done[1], (term | trunc).float())
    assert (col.rew[0] == 0).all() and float(col.ep_count) == 2.0
    assert _biteq(col.ep_sum, log[0:8] * torch.where(torch.arange(8, device="cuda") < 6, 2.0, 1.0))
    col.reset_tally()
    assert (col.ep_sum == 0).all() and float(col.ep_count) == 0.0


def test_rover_descriptors_are_refused():
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd import lift_rollout as LR
    from rollout_helpers import make_nets
    tr = _make_trainer()
    actor, critic = make_nets(2)
    with pytest.raises(_lib.RoverHipError, match="code 4"):       # ROVER_ERR_UNSUPPORTED
        LR.lift_rollout_act(actor, critic, torch.zeros(2, device="cuda"), _rows(4), 0, LR.default_hparams(), tr.state_scaler)
    with pytest.raises(_lib.RoverHipError, match="code 4"):       # the lift critic as the actor's partner, the rover's critic
        LR.lift_rollout_act(tr.actor, critic, tr.log_std, _rows(4), 0, LR.default_hparams(), tr.state_scaler)


def test_minibatch_on_the_collectors_rows_has_ratio_one(trainer):
    """Old and new log-probabilities come from one formula: FusedLiftPPO.minibatch on unchanged parameters re-evaluates the
    collector's rows to a KL entry ((r - 1) - log r averaged) of exactly 0, and to the collector's mean and raw value."""
    from isaac_rover_orbit_amd import lift_rollout as LR
    n, T = 33, 2
    col = LR.LiftRolloutCollector(trainer, n, T)
    raw_val = torch.empty(T, n, 1, device="cuda")
    for t in range(T):
        o = _rows(n, seed=20 + t)
        col.act(t, o)
        raw_val[t] = _run(trainer, o, counter=t, outs=(), value_scaler=False)["val"]
    B = T * n
    flat = lambda x: x.reshape(B, *x.shape[2:]).contiguous()      # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(3)
    adv, ret = torch.randn(B, device="cuda", generator=g), torch.randn(B, device="cuda", generator=g)
    idx = torch.randperm(B, device="cuda", generator=g)
    mean_out, value_out = torch.empty(B, A, device="cuda"), torch.empty(B, 1, device="cuda")
    stats = trainer.minibatch(flat(col.obs), flat(col.actions), flat(col.logp), flat(col.val), ret, adv, idx, train_scaler=False,
                              mean_out=mean_out, value_out=value_out)
    torch.cuda.synchronize()
    assert float(stats[0]) == 0.0
    assert _biteq(mean_out, flat(col.mean)[idx]) and _biteq(value_out, flat(raw_val)[idx])


def test_collector_drives_the_env_and_the_update():
    """A short rollout on the real env, the collector's tensors straight into gae / update, the tally against the torch lines."""
    from isaac_rover_orbit_amd import lift_ppo as LP
    from isaac_rover_orbit_amd import lift_rollout as LR
    from isaac_rover_orbit_amd.envs.lift_env import FrankaCubeLiftEnv, LiftEnvCfg
    n, T = 64, 6
    cfg = LiftEnvCfg(); cfg.scene.num_envs = n; cfg.seed = 1; cfg.log_reduction = "every_step"
    env = FrankaCubeLiftEnv(cfg)
    torch.manual_seed(0)
    tr = LP.FusedLiftPPO(LP.LiftMLP(LP.ACT_DIM, log_std=True).state_dict(), LP.LiftMLP(1).state_dict(), lr=1e-4)
    col = LR.LiftRolloutCollector(tr, n, T)
    obs, _ = env.reset()
    o = obs["policy"].clone()
    ep_sum, ep_count = torch.zeros(8, device="cuda"), torch.zeros((), device="cuda")
    for t in range(T):
        obs, rew, term, trunc, _ = env.step(col.act(t, o))
        o = obs["policy"]
        col.record(t, rew, term, trunc, env._log)
        k = env._log[8]
        ep_sum += torch.where(k > 0, env._log[0:8] * torch.where(torch.arange(8, device="cuda") < 6, k, 1.0), 0.0)
        ep_count += k
        assert _biteq(col.rew[t], rew * tr.hp.reward_scale) and _biteq(col.done[t], (term | trunc).float())
    assert col.counter == T and _biteq(col.ep_sum, ep_sum) and float(col.ep_count) == float(ep_count)
    for buf in (col.obs, col.actions, col.mean, col.logp, col.val, col.rew, col.done):
        assert buf.is_contiguous() and torch.isfinite(buf).all()
    adv, ret = tr.gae(col.rew, col.done, col.val, col.last_value(o))
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    val_s = tr.standardize(col.val.reshape(-1, 1).contiguous(), "value", train=True).reshape(T, n)
    ret_s = tr.standardize(ret.reshape(-1, 1).contiguous(), "value", train=True).reshape(T, n)
    kls, lr = tr.update(col.obs, col.actions, col.logp, val_s, ret_s, adv, epochs=2, minibatches=4)
    assert all(np.isfinite(k) for k in kls) and lr > 0 and torch.isfinite(tr.params).all()
    env.close()


def test_example_runs_with_the_fused_rollout(tmp_path):
    out = tmp_path / "stats.jsonl"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "05_train_lift.py"), "--rollout", "fused", "--update", "fused",
                        "--iterations", "2", "--num_envs", "96", "--rollouts", "4", "--out", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    assert len(lines) == 2 and all(np.isfinite(l["kl"]) and np.isfinite(l["mean_step_reward"]) and l["lr"] > 0 for l in lines)
    assert all({"iteration", "episodes", "kl_epochs", "stopped_epochs_total", "rollout_s", "update_s", "iteration_s"} <= set(l) for l in lines)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "05_train_lift.py"), "--rollout", "fused", "--iterations", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "requires --update fused" in r.stderr        # argparse refuses the pair before anything runs
