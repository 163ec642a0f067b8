"""The fused rollout step on the MI355X (include/rover_rollout.h, isaac_rover_orbit_amd.rollout) against its specification.

Inputs are rows of a stepped RoverEnv (ray misses are -inf there) with -inf / +inf / NaN injected at chosen rows and columns.

  * obs_out, mean_out, val_out, env_act: BIT-EXACT against torch.nan_to_num, policy.forward_pair on the sanitised rows, act.clamp
  * eps against TorchRollout's float64 Box-Muller over 2**19 draws: EPS_TOL below (four times the measured maximum, <= 1e-5)
  * act against mean + exp(ls) * eps in float64: 4 ulp of max(|mean|, |std * eps|)  (one expf, one multiply, one add)
  * logp against the float64 formula on the returned act / mean: 8 * 2**-23 * sum_c (0.5 x_c**2 + |ls_c| + 0.919)
  * shard invariance, counter determinism, the checkpoint, NULL optional outputs, and a 60-step rollout feeding FusedPPO
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import random_policy_weights, small_procedural
from ppo_reference import load_example
from rollout_helpers import _biteq, _inject, _run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23
# Largest |eps_kernel - eps_float64| measured on the MI355X over the 2**19 draws of test_eps_against_the_float64_spec
# (4096 rows x 64 counters x one pair, seed 42; largest |eps| among them 4.789): 5.117e-07, about one ulp at |eps| in [4, 8).
# The bound is four times that, 2.05e-06, and stays below the ceiling of 1e-5 (about 20 ulp at the largest possible
# |eps| = 5.77) the contract allows.
EPS_MEASURED_MAX = 5.117e-07
EPS_TOL = 4.0 * EPS_MEASURED_MAX
assert EPS_TOL <= 1e-5
SIZES = [1, 15, 16, 17, 4096, 4099]


@pytest.fixture(scope="module")
def nets():
    from isaac_rover_orbit_amd.policy import RoverNet
    wa, ba = random_policy_weights(seed=21, out_dim=2, scale=3.0)
    wc, bc = random_policy_weights(seed=22, out_dim=1, scale=3.0)
    return RoverNet(wa, ba, n_enc=2, final_act="tanh"), RoverNet(wc, bc, n_enc=2, final_act="none")


@pytest.fixture(scope="module")
def env_rows():
    """(4608, 965) raw observation rows of a RoverEnv after five random steps (misses are -inf), on the GPU."""
    from isaac_rover_orbit_amd.cfg import RoverEnvCfg
    from isaac_rover_orbit_amd.envs import RoverEnv
    n = 4608
    ter = small_procedural()
    ter.make_spawns(2 * n)
    cfg = RoverEnvCfg(); cfg.scene.num_envs = n; cfg.terrain.kind = "custom"
    env = RoverEnv(cfg, terrain=ter)
    obs, _ = env.reset()
    g = torch.Generator(device="cuda").manual_seed(3)
    for _ in range(5):
        obs, *_ = env.step(torch.rand(n, 2, device="cuda", generator=g) * 2 - 1)
    rows = obs["policy"].clone()
    env.close()
    return rows


@pytest.mark.parametrize("n", SIZES)
def test_outputs_against_the_spec(nets, env_rows, n):
    from isaac_rover_orbit_amd import rollout as R
    from isaac_rover_orbit_amd.policy import forward_pair
    raw = _inject(env_rows, n)
    assert not torch.isfinite(raw).all()
    log_std = torch.tensor([0.1, -0.7], device="cuda")
    o = _run(nets, raw, log_std, counter=5, env_id_offset=11)
    clean = torch.nan_to_num(raw, nan=0.0, posinf=R.FLT_MAX, neginf=0.0)
    assert _biteq(o["obs"], clean) and torch.isfinite(o["obs"]).all() and (o["obs"][:, 964] == R.FLT_MAX).any()
    mean, val = forward_pair(nets[0], nets[1], clean)
    assert _biteq(o["mean"], mean) and _biteq(o["val"], val) and torch.isfinite(mean).all() and torch.isfinite(val).all()
    assert _biteq(o["env_act"], o["act"].clamp(-1.0, 1.0))
    assert (o["act"].abs() > 1.0).any() or n < 16                                      # the clamp does something
    o2 = _run(nets, raw, log_std, counter=5, env_id_offset=11, clip_actions=0)
    assert _biteq(o2["env_act"], o2["act"]) and _biteq(o2["act"], o["act"])
    # eps, act, logp against float64
    eps64 = R.standard_normals(42, 11 + np.arange(n), 5, 2)
    eps = o["eps"].cpu().numpy().astype(np.float64)
    d_eps = np.abs(eps - eps64).max()
    m, a = o["mean"].cpu().numpy().astype(np.float64), o["act"].cpu().numpy().astype(np.float64)
    ls = log_std.cpu().numpy().astype(np.float64)
    noise = np.exp(ls) * eps
    d_act = np.abs(a - (m + noise)) / np.maximum(np.abs(m), np.abs(noise))
    x = (a - m) / np.exp(ls)
    want = (-0.5 * x * x - ls - 0.9189385332).sum(1)
    scale = (0.5 * x * x + np.abs(ls) + 0.919).sum(1)
    d_lp = np.abs(o["logp"].cpu().numpy().astype(np.float64) - want) / scale
    print(f"n={n}: |eps - spec| {d_eps:.3e}; act {d_act.max() / ULP:.2f} ulp; logp {d_lp.max() / ULP:.2f} ulp of the bound's scale")
    assert d_eps <= EPS_TOL
    assert d_act.max() <= 4 * ULP
    assert d_lp.max() <= 8 * ULP


def test_eps_against_the_float64_spec(nets, env_rows):
    """The 2**19 draws of tests/test_rollout.py::test_draw_statistics_seed_42 (4096 rows x 64 counters x one pair, seed 42)."""
    from isaac_rover_orbit_amd import rollout as R
    raw = torch.nan_to_num(env_rows[:4096], neginf=0.0)
    log_std = torch.zeros(2, device="cuda")
    worst, biggest = 0.0, 0.0
    for k in range(64):
        eps = _run(nets, raw, log_std, counter=k, outs=("eps",))["eps"].cpu().numpy().astype(np.float64)
        ref = R.standard_normals(42, np.arange(4096), k, 2)
        worst, biggest = max(worst, float(np.abs(eps - ref).max())), max(biggest, float(np.abs(ref).max()))
    print(f"max |eps_kernel - eps_float64| over 2**19 draws = {worst:.3e} (largest |eps| {biggest:.3f}); bound {EPS_TOL:.3e}")
    assert worst <= EPS_TOL


def test_logp_and_act_at_both_log_std_clamps(nets, env_rows):
    """log_std above the upper clamp (std = e**2) and below the lower one (std = e**-20: the noise mostly rounds away, and the
    log-probability is that of the STORED action, as the update will recompute it)."""
    n = 4099
    raw = _inject(env_rows, n)
    for raw_ls, ls in (((5.0, -30.0), (2.0, -20.0)), ((-30.0, 2.0), (-20.0, 2.0)), ((-20.0, 2.0), (-20.0, 2.0))):
        o = _run(nets, raw, torch.tensor(raw_ls, device="cuda"), counter=9)
        ls = np.array(ls, dtype=np.float64)
        eps, m, a = (o[k].cpu().numpy().astype(np.float64) for k in ("eps", "mean", "act"))
        noise = np.exp(ls) * eps
        d_act = np.abs(a - (m + noise)) / np.maximum(np.abs(m), np.abs(noise))
        x = (a - m) / np.exp(ls)
        want = (-0.5 * x * x - ls - 0.9189385332).sum(1)
        scale = (0.5 * x * x + np.abs(ls) + 0.919).sum(1)
        d_lp = np.abs(o["logp"].cpu().numpy().astype(np.float64) - want) / scale
        print(f"log_std {raw_ls}: act {d_act.max() / ULP:.2f} ulp; logp {d_lp.max() / ULP:.2f} ulp of the bound's scale")
        assert np.isfinite(want).all() and torch.isfinite(o["logp"]).all()
        assert d_act.max() <= 4 * ULP
        assert d_lp.max() <= 8 * ULP


def test_shard_invariance(nets, env_rows):
    raw = _inject(env_rows, 4096)
    log_std = torch.tensor([0.2, -1.0], device="cuda")
    whole = _run(nets, raw, log_std, counter=3)
    lo = _run(nets, raw[:2048].contiguous(), log_std, counter=3, env_id_offset=0)
    hi = _run(nets, raw[2048:].contiguous(), log_std, counter=3, env_id_offset=2048)
    for k in whole:
        assert _biteq(whole[k], torch.cat([lo[k], hi[k]])), k


def test_counter_determinism(nets, env_rows):
    raw = _inject(env_rows, 4099)
    log_std = torch.tensor([0.2, -1.0], device="cuda")
    a, b, c = _run(nets, raw, log_std, counter=7), _run(nets, raw, log_std, counter=7), _run(nets, raw, log_std, counter=8)
    for k in a:
        assert _biteq(a[k], b[k]), k
    assert (a["eps"] != c["eps"]).all()
    for k in ("obs", "mean", "val"):
        assert torch.equal(a[k], c[k]), k
    big = _run(nets, raw, log_std, counter=7 + 2 ** 32)                               # the high counter word is part of the input
    assert (a["eps"] != big["eps"]).all()


def test_null_optional_outputs(nets, env_rows):
    raw = _inject(env_rows, 4099)
    log_std = torch.tensor([0.2, -1.0], device="cuda")
    full = _run(nets, raw, log_std, counter=2)
    for outs in (("obs",), ("act",), ("env_act",), ("logp",), ("eps",), ("act", "logp"), ("obs", "env_act", "eps"), ()):
        part = _run(nets, raw, log_std, counter=2, outs=outs)
        for k in part:
            assert _biteq(part[k], full[k]), (outs, k)
    # the all-NULL form is the bootstrap-value call: the value of forward_pair, nothing else
    from isaac_rover_orbit_amd import rollout as R
    from isaac_rover_orbit_amd.policy import forward_pair
    col = R.RolloutCollector(nets[0], nets[1], log_std, 4099, 2)
    v = col.last_value(raw)
    assert col.counter == 0
    assert torch.equal(v, forward_pair(nets[0], nets[1], torch.nan_to_num(raw, nan=0.0, posinf=R.FLT_MAX, neginf=0.0))[1][:, 0])


def test_collector_slots_record_and_checkpoint(nets, env_rows):
    from isaac_rover_orbit_amd import rollout as R
    n, T = 4099, 3
    raw = _inject(env_rows, n)
    log_std = torch.tensor([0.2, -1.0], device="cuda")
    col = R.RolloutCollector(nets[0], nets[1], log_std, n, T, seed=(5 << 32) | 9, env_id_offset=64)
    ea0 = col.act(0, raw).clone()
    ea1 = col.act(1, {"policy": raw}).clone()
    assert col.counter == 2 and not torch.equal(ea0, ea1)
    ref = _run(nets, raw, log_std, counter=1, seed_lo=9, seed_hi=5, env_id_offset=64)
    for k, buf in (("obs", col.obs), ("mean", col.mean), ("act", col.actions), ("logp", col.logp)):
        assert torch.equal(buf[1], ref[k]), k
    assert torch.equal(col.val[1], ref["val"][:, 0]) and torch.equal(ea1, ref["env_act"])
    assert (col.obs[2] == 0).all()                                                     # slot 2 untouched
    g = torch.Generator(device="cuda").manual_seed(1)
    rew = torch.randn(n, device="cuda", generator=g)
    term, trunc = torch.rand(n, device="cuda", generator=g) < 0.3, torch.rand(n, device="cuda", generator=g) < 0.3
    col.record(1, rew, term, trunc)
    assert torch.equal(col.rew[1], rew) and torch.equal(col.done[1], (term | trunc).float())
    assert (col.rew[0] == 0).all() and (col.done[2] == 0).all()
    # the checkpoint is the counter: a fresh collector continues with the original's bits
    fresh = R.RolloutCollector(nets[0], nets[1], log_std, n, T)
    fresh.load_state_dict(col.state_dict())
    assert fresh.state_dict() == {"seed": (5 << 32) | 9, "counter": 2, "env_id_offset": 64}
    assert torch.equal(col.act(2, raw), fresh.act(2, raw))
    for a, b in ((col.actions, fresh.actions), (col.logp, fresh.logp), (col.mean, fresh.mean), (col.val, fresh.val), (col.obs, fresh.obs)):
        assert torch.equal(a[2], b[2])
    # ... and equals the CPU specification within the eps bound (same seed, ids and counter)
    spec = R.TorchRollout(lambda o: col.mean[2].cpu(), lambda o: col.val[2].cpu(), log_std.cpu(), n, T)
    spec.load_state_dict({"seed": (5 << 32) | 9, "counter": 2, "env_id_offset": 64})
    spec.act(2, raw.cpu())
    assert torch.equal(spec.obs[2], col.obs[2].cpu())
    assert (spec.actions[2] - col.actions[2].cpu()).abs().max() <= 4 * EPS_TOL
    with pytest.raises(ValueError):
        col.act(0, raw[:100])
    with pytest.raises(ValueError):
        col.record(0, rew.double(), term, trunc)


def test_rollout_feeds_the_fused_ppo_update():
    """60 steps at 4096 envs on FusedPPO's own networks; gae and update take the collector's tensors as they are; the first act of
    the next rollout runs on the updated parameters."""
    from isaac_rover_orbit_amd import rollout as R
    from isaac_rover_orbit_amd.cfg import RoverEnvCfg
    from isaac_rover_orbit_amd.envs import RoverEnv
    from isaac_rover_orbit_amd.policy import forward_pair
    from isaac_rover_orbit_amd.ppo import FusedPPO
    ex = load_example()
    torch.manual_seed(0)
    pol, val = ex.Net(2, True), ex.Net(1, False)
    fused = FusedPPO(pol.state_dict(), val.state_dict(), lr=1e-4)
    n, T = 4096, 60
    ter = small_procedural()
    ter.make_spawns(2 * n)
    cfg = RoverEnvCfg(); cfg.scene.num_envs = n; cfg.terrain.kind = "custom"
    env = RoverEnv(cfg, terrain=ter)
    col = R.RolloutCollector(fused.actor, fused.critic, fused.log_std, n, T)
    obs, _ = env.reset()
    o = obs["policy"]
    for t in range(T):
        obs, rew, term, trunc, _ = env.step(col.act(t, o))
        o = obs["policy"]
        col.record(t, rew, term, trunc)
    assert col.counter == T
    for buf in (col.obs, col.actions, col.mean, col.logp, col.val, col.rew, col.done):
        assert buf.is_contiguous() and torch.isfinite(buf).all()
    assert float(col.done.sum()) >= 0 and set(col.done.unique().tolist()) <= {0.0, 1.0}
    p0 = fused.params.clone()
    adv, ret = fused.gae(col.rew, col.done, col.val, col.last_value(o))
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    kls, _ = fused.update(col.obs, col.actions, col.logp, col.val, ret, adv)
    assert all(np.isfinite(k) for k in kls) and np.isfinite(fused.lr)
    assert torch.isfinite(fused.params).all() and not torch.equal(fused.params, p0)
    first = col.act(0, o).clone()
    clean = torch.nan_to_num(o, nan=0.0, posinf=R.FLT_MAX, neginf=0.0)
    mean, v = forward_pair(fused.actor, fused.critic, clean)
    assert torch.equal(col.mean[0], mean) and torch.equal(col.val[0], v[:, 0]) and col.counter == T + 1
    ls = fused.log_std.clamp(-20.0, 2.0)
    assert not torch.equal(ls, torch.zeros_like(ls))                                    # the update moved log_std as well ...
    x = (col.actions[0] - mean) / ls.exp()                                              # ... and the collector read the new one
    assert torch.allclose(col.logp[0], (-0.5 * x * x - ls - 0.9189385332).sum(1), rtol=1e-5, atol=1e-5)
    assert torch.equal(first, col.actions[0].clamp(-1.0, 1.0))
    env.close()


def test_example_runs_with_the_fused_rollout(tmp_path):
    out = tmp_path / "stats.jsonl"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "04_train_ppo.py"), "--rollout", "fused", "--update", "fused",
                        "--iterations", "2", "--num_envs", "512", "--out", str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    assert len(lines) == 2 and all(np.isfinite(l["kl"]) and np.isfinite(l["mean_step_reward"]) and l["lr"] > 0 for l in lines)
