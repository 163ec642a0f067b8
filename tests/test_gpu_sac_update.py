"""Fused SAC (include/rover_sac.h) against the float64 torch spec: the fused error stays within a small multiple of torch
fp32's error on the same inputs (td3_helpers.check: 4x plus a 1e-5 floor).  Critic step (y with its entropy term, both critics'
gradients, Adam), policy step (u, logp, dL/dmu, the actor and log_std gradients, Adam, the entropy step, the replicas), the
log_std clamp mask, ties of the two critics, learn_entropy off, Polyak bit for bit, 20 updates at ragged sizes, stale
workspace, repeatability, bad indices, no host synchronisation and the example.

Every input is made on the CPU (networks, memory, indices, draws) and copied to the device, so the seeds of the ragged runs,
picked with TorchSAC in float64 on the CPU, name the same run here."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from sac_helpers import check, draws, fill, grads, nets, params, poison_ws, sample, trainers, update_with_margin

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
TRAINER_VECTORS = ("params", "target", "grad", "adam_m", "adam_v", "state", "rep_a")


def memory(seed, M=4, N=64, steps=6):
    """td3_helpers.fill on the CPU (its draws depend on the generator's device), copied to the GPU."""
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    cpu = ReplayMemory(M, N, device="cpu")
    fill(cpu, steps, seed=seed)
    mem = ReplayMemory(M, N, device=DEV)
    for name in ("obs", "actions", "rewards", "terminated", "ring_pos"):
        getattr(mem, name).copy_(getattr(cpu, name))
    mem.memory_index, mem.filled, mem.cursor = cpu.memory_index, cpu.filled, cpu.cursor
    return mem


def setup(seed=0, bias=None, log_std=None, tie=False, **hp):
    mods = nets(seed, "cpu", bias=bias, log_std=log_std)
    if tie:
        mods[2].load_state_dict(mods[1].state_dict())
    mods = [m.to(DEV) for m in mods]
    fused, specs = trainers(mods, **hp)
    return memory(seed + 1), fused, specs


def indices(mem, n, seed):
    return torch.randint(0, len(mem), (n,), generator=torch.Generator().manual_seed(seed)).to(DEV)


def critic_case(mem, fused, specs, idx, eps):
    """One critic step on every path; returns the fused y and {dtype: (y, grads c1, grads c2, stats)}."""
    y = torch.empty(idx.numel(), device=DEV)
    fused.critic_step(mem, idx, eps, y_out=y)
    out = {}
    for dt, sp in specs.items():
        st = sp.critic_step(*sample(mem, idx, dt), eps[:, 0:2])
        out[dt] = (st["y"].reshape(-1), grads(sp.critic_1), grads(sp.critic_2), st)
    return y, out


def policy_case(mem, fused, specs, idx, eps):
    """One policy step on every path; returns the fused debug outputs and {dtype: dict of the spec's u, logp, dL/dmu, gradients}."""
    from isaac_rover_orbit_amd.sac import gaussian_act
    n = idx.numel()
    got = {"u": torch.empty(n, 2, device=DEV), "logp": torch.empty(n, device=DEV), "dmean": torch.empty(n, 2, device=DEV)}
    fused.policy_step(mem, idx, eps, u_out=got["u"], logp_out=got["logp"], dmean_out=got["dmean"])
    out = {}
    for dt, sp in specs.items():
        s = sample(mem, idx, dt)[0]
        seen = {}

        def hook(_, inp, o, seen=seen):
            o.retain_grad()
            seen["mu"] = o
        h = sp.policy.mlp[-1].register_forward_hook(hook)
        log_std = sp.policy.log_std_parameter.detach().clone()
        st = sp.policy_step(s, eps[:, 2:4])
        h.remove()
        u, logp = gaussian_act(seen["mu"].detach(), log_std, eps[:, 2:4].to(dt))
        out[dt] = {"u": u, "logp": logp.reshape(-1), "dmean": seen["mu"].grad, "grad": grads(sp.policy), "stats": st,
                   "x": seen["mu"].detach() + log_std.clamp(-20, 2).exp() * eps[:, 2:4].to(dt)}
    return got, out


def check_policy_params(fused, specs):
    p = fused.unvector(fused.params)
    s64, s32 = specs[F64], specs[F32]
    check(p["policy"], params(s64.policy), params(s32.policy), what="policy ")
    check(p["log_entropy_coefficient"], s64.log_entropy_coefficient.detach().reshape(1), s32.log_entropy_coefficient.detach().reshape(1),
          what="log_alpha")


def test_critic_step_with_both_clamps_hit():
    from isaac_rover_orbit_amd.sac import gaussian_act
    mem, fused, specs = setup(seed=0, bias=(1.5, -1.5))
    n = 512
    idx, eps = indices(mem, n, 7), draws(n, 8).to(DEV)
    s64 = specs[F64]
    with torch.no_grad():
        s2 = sample(mem, idx, F64)[3]
        mu = s64.policy(s2)
        x = mu + eps[:, 0:2].double()                      # log_std = 0: sigma = 1
        u2, logp2 = gaussian_act(mu, s64.policy.log_std_parameter, eps[:, 0:2].double())
    assert bool((x > 1).any()) and bool((x < -1).any()) and bool((x.abs() < 1).any())
    assert bool((u2 == 1).any()) and bool((u2 == -1).any()) and float(logp2.abs().min()) > 0.1
    y, out = critic_case(mem, fused, specs, idx, eps)
    r64, r32 = out[F64], out[F32]
    check(y, r64[0], r32[0], what="y")
    g = fused.unvector(fused.grad)
    check(g["critic_1"], r64[1], r32[1], what="grad c1 ")
    check(g["critic_2"], r64[2], r32[2], what="grad c2 ")
    p = fused.unvector(fused.params)
    for k in ("critic_1", "critic_2"):
        check(p[k], params(getattr(specs[F64], k)), params(getattr(specs[F32], k)), what=f"{k} ")
    st = fused.stats()
    assert st["critic_step"] == 1 and st["actor_step"] == 0 and st["entropy_step"] == 0 and st["bad_index"] == 0
    for k in ("y_mean", "q1_mean", "q2_mean", "critic_loss"):
        assert st[k] == pytest.approx(r64[3][k], rel=1e-3, abs=1e-6), k
    # nothing but the critic blocks moved
    assert torch.equal(fused.params[:fused.n_a], fused.rep_a[:fused.n_a]) and not bool(fused.grad[:fused.n_a].any())
    assert not bool(fused.grad[fused.tail:].any())


def test_policy_step_entropy_step_and_replicas():
    """stats()["alpha"] is the coefficient the step used, formed on the device as (float)exp((double)log_alpha) from
    log_alpha = log(float32(0.2)): that is 0.19999999, one float32 ulp below 0.2f (no float32 log_alpha maps to 0.2f), so the
    test asserts that exact value and that it is within one ulp of 0.2f -- not the stepped coefficient, which is 0.5 % away."""
    mem, fused, specs = setup(seed=4, bias=(1.5, -1.5))
    n = 512
    idx, eps = indices(mem, n, 10), draws(n, 11).to(DEV)
    critic_case(mem, fused, specs, idx, eps)
    la0 = fused.log_alpha.clone()
    got, out = policy_case(mem, fused, specs, idx, eps)
    r64, r32 = out[F64], out[F32]
    x = r64["x"]
    assert bool((x > 1).any()) and bool((x < -1).any()) and bool((x.abs() < 1).any())
    for k in ("u", "logp", "dmean"):
        check(got[k], r64[k], r32[k], what=k)
    g = fused.unvector(fused.grad)["policy"]
    check(g, r64["grad"], r32["grad"], what="policy grad ")
    assert float(r64["grad"]["log_std_parameter"].abs().min()) > 0
    check(g["log_std_parameter"], r64["grad"]["log_std_parameter"], r32["grad"]["log_std_parameter"], what="log_std grad")
    check_policy_params(fused, specs)
    assert not torch.equal(fused.log_alpha, la0)
    st = fused.stats()
    assert (st["critic_step"], st["actor_step"], st["entropy_step"], st["bad_index"]) == (1, 1, 1, 0)
    alpha0 = np.float32(np.exp(np.float64(np.log(np.float32(0.2)))))
    assert st["alpha"] == float(alpha0) and abs(float(alpha0) - float(np.float32(0.2))) <= float(np.spacing(np.float32(0.2)))
    for k in ("policy_loss", "logp_mean", "entropy_loss"):
        assert st[k] == pytest.approx(r64["stats"][k], rel=1e-3, abs=1e-6), k
    # the gradient's padding is exact zeros
    tail = fused.grad[fused.tail:]
    assert not bool(tail[2:4].any()) and not bool(tail[5:].any()) and bool(tail[4] != 0)
    # the replicas .actor reads are the parameters after Adam
    obs = mem.gather(idx)[0]
    with torch.no_grad():
        ref64, ref32 = specs[F64].policy(obs.double()), specs[F32].policy(obs)
    check(fused.actor(obs), ref64, ref32, what="actor(obs)")
    rep = fused.rep_a.view(fused.n_copies, -1)
    assert all(torch.equal(rep[c], fused.params[:fused.n_a]) for c in range(fused.n_copies))
    assert fused.log_std.data_ptr() == fused.params.data_ptr() + 4 * fused.tail


def test_log_std_outside_its_clamp_gets_no_gradient():
    mem, fused, specs = setup(seed=5, log_std=(2.5, -1.0))
    n = 512
    idx, eps = indices(mem, n, 12), draws(n, 13).to(DEV)
    critic_case(mem, fused, specs, idx, eps)
    t = fused.tail
    before = [v[t:t + 2].clone() for v in (fused.params, fused.adam_m, fused.adam_v)]
    got, out = policy_case(mem, fused, specs, idx, eps)
    assert float(fused.grad[t]) == 0.0 and float(out[F64]["grad"]["log_std_parameter"][0]) == 0.0
    for v, b in zip((fused.params, fused.adam_m, fused.adam_v), before):
        assert torch.equal(v[t:t + 1].view(torch.int32), b[0:1].view(torch.int32))
        assert not torch.equal(v[t + 1:t + 2], b[1:2])                                  # component 1 moves
    assert float(fused.params[t]) == 2.5
    for k in ("u", "logp", "dmean"):
        check(got[k], out[F64][k], out[F32][k], what=k)
    check_policy_params(fused, specs)


def test_ties_of_the_two_critics_split_the_gradient():
    mem, fused, specs = setup(seed=6, bias=(1.5, -1.5), tie=True)
    n = 512
    idx, eps = indices(mem, n, 14), draws(n, 15).to(DEV)
    critic_case(mem, fused, specs, idx, eps)
    b = fused.blocks(fused.params)
    assert torch.equal(b["critic_1"], b["critic_2"])                                    # the same y keeps the twins equal
    s64 = specs[F64]
    assert all(torch.equal(p, q) for p, q in zip(s64.critic_1.parameters(), s64.critic_2.parameters()))
    got, out = policy_case(mem, fused, specs, idx, eps)
    check(got["dmean"], out[F64]["dmean"], out[F32]["dmean"], what="dmean")
    check(fused.unvector(fused.grad)["policy"], out[F64]["grad"], out[F32]["grad"], what="policy grad ")


def test_learn_entropy_off_never_steps_log_alpha():
    mem, fused, specs = setup(seed=7, learn_entropy=False)
    n = 256
    la0 = fused.params[fused.tail + 4:fused.tail + 8].clone()
    for i in range(2):
        idx, eps = indices(mem, n, 16 + i), draws(n, 18 + i).to(DEV)
        fused.update(mem, idx, eps)
        for sp in specs.values():
            sp.update(mem, idx, eps)
    t = fused.tail
    for v in (fused.params, ):
        assert torch.equal(v[t + 4:t + 8].view(torch.int32), la0.view(torch.int32))
    assert not bool(fused.adam_m[t + 4:t + 8].any()) and not bool(fused.adam_v[t + 4:t + 8].any()) and float(fused.grad[t + 4]) == 0.0
    st = fused.stats()
    assert (st["critic_step"], st["actor_step"], st["entropy_step"]) == (2, 2, 0)
    assert st["alpha"] == float(np.float32(np.exp(np.float64(np.log(np.float32(0.2))))))
    check_policy_params(fused, specs)


def test_polyak_is_bit_identical_to_torch_fp32_and_writes_nothing_else():
    mem, fused, _ = setup(seed=8)
    n = 256
    idx, eps = indices(mem, n, 20), draws(n, 21).to(DEV)
    fused.critic_step(mem, idx, eps)
    count = 2 * fused.n_c
    buf = torch.cat([fused.target, torch.full((64,), 1234.5, device=DEV)])
    fused.target = buf[:count]
    assert fused.target.data_ptr() % 16 == 0
    tgt, p = fused.target.clone(), fused.params[fused.n_a:fused.n_a + count].clone()
    assert not torch.equal(tgt, p)
    everything_else = [v.clone() for v in (fused.params, fused.grad, fused.adam_m, fused.adam_v, fused.state)]
    fused.polyak()
    tgt.mul_(1 - 0.005)
    tgt.add_(0.005 * p)
    assert torch.equal(fused.target.view(torch.int32), tgt.view(torch.int32))
    assert bool((buf[count:] == 1234.5).all())
    for v, b in zip((fused.params, fused.grad, fused.adam_m, fused.adam_v, fused.state), everything_else):
        assert torch.equal(v, b)


# seeds picked with TorchSAC in float64 on the CPU among 0 .. 31 (the margin below over all 20 updates: 8.4e-4 at n = 70 with
# seed 19, 1.3e-4 at n = 384 with seed 20); 70 is short of the 256-row block and no multiple of the 64-row dense tile, 384 is
# short of the 512-row chunk and more than one block
@pytest.mark.parametrize("n,seed", [(70, 19), (384, 20)])
def test_twenty_updates_at_ragged_sizes_track_the_float64_spec(n, seed):
    mem, fused, specs = setup(seed=seed)
    g = torch.Generator().manual_seed(100 + seed)
    margin = math.inf
    for step in range(20):
        idx = torch.randint(0, len(mem), (n,), generator=g).to(DEV)
        eps = draws(n, 1000 * seed + step).to(DEV)
        fused.update(mem, idx, eps)
        margin = min(margin, update_with_margin(specs[F64], mem, idx, eps))
        specs[F32].update(mem, idx, eps)
    # no clamp (| |x| - 1 |) and no min (| q1 - q2 |) decision of any row and step lies within 1e-4 of flipping: a flip between
    # precisions would be a discontinuity, not an error
    assert margin >= 1e-4, margin
    st = fused.stats()
    assert (st["critic_step"], st["actor_step"], st["entropy_step"], st["bad_index"]) == (20, 20, 20, 0)
    p, t = fused.unvector(fused.params), fused.unvector(fused.target)
    s64, s32 = specs[F64], specs[F32]
    for k in ("policy", "critic_1", "critic_2"):
        check(p[k], params(getattr(s64, k)), params(getattr(s32, k)), what=f"{k} ")
    for k in ("critic_1", "critic_2"):
        check(t[k], params(getattr(s64, "target_" + k)), params(getattr(s32, "target_" + k)), what=f"target_{k} ")
    check(p["log_entropy_coefficient"], s64.log_entropy_coefficient.detach().reshape(1), s32.log_entropy_coefficient.detach().reshape(1),
          what="log_alpha")


def same_trainer(a, b):
    for name in TRAINER_VECTORS:
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x, y) and torch.equal(x.view(torch.int32), y.view(torch.int32)), name


def test_stale_workspace_and_repeatability():
    from isaac_rover_orbit_amd.sac import FusedSAC
    mods = [m.to(DEV) for m in nets(9, "cpu", bias=(1.0, -1.0))]
    mem = memory(10)
    a, b, c = (FusedSAC(*(m.state_dict() for m in mods)) for _ in range(3))
    n = 300
    poison_ws(b, n)                                        # every float of b's workspace is a NaN
    for i in range(2):
        idx, eps = indices(mem, n, 22 + i), draws(n, 24 + i).to(DEV)
        for f in (a, b, c):
            f.update(mem, idx, eps)
            if f is b:
                poison_ws(b, n)
    same_trainer(a, b)
    same_trainer(a, c)
    assert bool(torch.isfinite(a.params).all()) and bool(torch.isfinite(a.grad).all())


def test_bad_index_is_sticky():
    mem, fused, _ = setup(seed=11)
    n = 64
    eps = draws(n, 26).to(DEV)
    idx = indices(mem, n, 27)
    fused.update(mem, idx, eps)
    assert fused.stats()["bad_index"] == 0
    bad = idx.clone()
    bad[5] = len(mem)                                      # one past the filled rows
    fused.critic_step(mem, bad, eps)
    assert fused.stats()["bad_index"] == 1
    fused.update(mem, idx, eps)
    assert fused.stats()["bad_index"] == 1 and bool(torch.isfinite(fused.params).all())
    bad[5] = -1
    fused2 = setup(seed=11)[1]
    fused2.policy_step(mem, bad, eps)
    assert fused2.stats()["bad_index"] == 1


def test_update_does_not_synchronise_and_arguments_are_checked():
    mem, fused, _ = setup(seed=12)
    n = 128
    idx, eps = indices(mem, n, 28), draws(n, 29).to(DEV)
    fused.update(mem, idx, eps)                            # the workspace is allocated here
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fused.update(mem, idx, eps)
        fused.update(mem, idx, eps)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    st = fused.stats()                                     # the one synchronisation
    assert st["critic_step"] == 3 and all(math.isfinite(st[k]) for k in ("critic_loss", "policy_loss", "entropy_loss", "alpha"))
    for bad_idx, bad_eps in ((idx.cpu(), eps), (idx.int(), eps), (idx, eps.cpu()), (idx, eps.double()), (idx, eps[:, :2].contiguous()),
                             (idx, eps[:-1]), (idx, eps.t().contiguous().t()), (idx[::2], eps[::2])):
        with pytest.raises(ValueError):
            fused.update(mem, bad_idx, bad_eps)
    with pytest.raises(ValueError):
        fused.critic_step(mem, idx, eps, y_out=torch.empty(n - 1, device=DEV))
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    with pytest.raises(ValueError):
        fused.update(ReplayMemory(4, 64, device=DEV), idx, eps)                        # empty


def test_checkpoint_round_trip_of_the_fused_trainer():
    from isaac_rover_orbit_amd.sac import CHECKPOINT_KEYS, FusedSAC
    mem, fused, _ = setup(seed=13)
    n = 64
    fused.update(mem, indices(mem, n, 30), draws(n, 31).to(DEV))
    ck = fused.state_dict()
    assert tuple(ck) == CHECKPOINT_KEYS and ck["log_entropy_coefficient"].shape == (1,) and "log_std_parameter" in ck["policy"]
    back = FusedSAC.from_checkpoint(ck)
    assert torch.equal(back.params, fused.params) and torch.equal(back.target, fused.target)
    assert not torch.equal(back.target, back.params[back.n_a:back.n_a + 2 * back.n_c])
    pol = nets(0)[0]
    pol.load_state_dict(ck["policy"])


def test_example_runs_with_the_fused_update(tmp_path):
    spec = importlib.util.spec_from_file_location("train_sac_example", os.path.join(ROOT, "examples", "09_train_sac.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out, save = tmp_path / "sac.jsonl", tmp_path / "sac.pt"
    ex.main(["--update", "fused", "--num_envs", "256", "--timesteps", "6", "--batch_size", "128", "--memory_size", "4", "--log_every", "3",
             "--random_timesteps", "1", "--learning_starts", "1", "--out", str(out), "--save", str(save)])
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    assert len(lines) == 2 and lines[-1]["timestep"] == 6 and lines[-1]["updates"] == 5
    assert (lines[-1]["critic_step"], lines[-1]["actor_step"], lines[-1]["entropy_step"], lines[-1]["bad_index"]) == (5, 5, 5, 0)
    for l in lines:
        assert all(math.isfinite(l[k]) for k in ex.LOGGED + ("env_steps_per_s",)), l
    assert lines[-1]["alpha"] != lines[0]["alpha"]
    ck = torch.load(save, map_location="cpu", weights_only=False)
    assert "log_entropy_coefficient" in ck and "target_policy" not in ck
