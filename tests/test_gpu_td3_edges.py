"""Fused TD3 at its edges: ragged row counts, a memory not yet filled, a wrapped memory, a ring past 2^31 floats sampled in its
last slots, an out-of-range index, run-to-run bit reproducibility and checkpoints that the torch modules load."""
import pytest
import torch

from td3_helpers import check, copies, fill, nets
from test_gpu_td3_update import DEV, grads, params, sample, setup

pytestmark = pytest.mark.gpu


def both_steps(mem, fused, specs, idx):
    """A critic step then an actor step on both paths; checks the gradients of all three networks and the parameters."""
    y = torch.empty(idx.numel(), device=DEV)
    fused.critic_step(mem, idx, y_out=y)
    gc = fused.unvector(fused.grad)
    fused.actor_step(mem, idx)
    ga = fused.unvector(fused.grad)["policy"]
    ref = {}
    for dt, sp in specs.items():
        st = sp.critic_step(*sample(mem, idx, dt))
        g1, g2 = grads(sp.critic_1), grads(sp.critic_2)
        sp.actor_step(sample(mem, idx, dt)[0])
        ref[dt] = (st["y"].reshape(-1), g1, g2, grads(sp.policy))
    r64, r32 = ref[torch.float64], ref[torch.float32]
    check(y, r64[0], r32[0], what="y")
    check(gc["critic_1"], r64[1], r32[1], what="grad c1 ")
    check(gc["critic_2"], r64[2], r32[2], what="grad c2 ")
    check(ga, r64[3], r32[3], what="grad actor ")
    p = fused.unvector(fused.params)
    for k in ("policy", "critic_1", "critic_2"):
        check(p[k], params(getattr(specs[torch.float64], k)), params(getattr(specs[torch.float32], k)), what=f"{k} ")
    assert fused.stats()["bad_index"] == 0


@pytest.mark.parametrize("n", [1, 63, 65, 4097])
def test_ragged_rows(n):
    mem, fused, specs = setup(seed=10, M=4, N=1100, steps=5)
    both_steps(mem, fused, specs, mem.sample_indices(n, torch.Generator(device=DEV).manual_seed(n)))


def test_memory_not_yet_filled():
    mem, fused, specs = setup(seed=11, M=8, N=64, steps=3)
    assert len(mem) == 3 * 64 and not mem.filled
    idx = mem.sample_indices(300, torch.Generator(device=DEV).manual_seed(1))
    assert int(idx.max()) < len(mem)
    both_steps(mem, fused, specs, idx)


def test_wrapped_memory():
    mem, fused, specs = setup(seed=12, M=3, N=64, steps=10)
    assert mem.filled and mem.cursor == 10 % 4
    # adds 7, 8, 9 hold memory slots 1, 2, 0 at ring slots 3, 0, 1: the positions wrapped past the last ring slot
    assert mem.ring_pos.tolist() == [1, 3, 0]
    both_steps(mem, fused, specs, mem.sample_indices(300, torch.Generator(device=DEV).manual_seed(2)))


def test_ring_past_two_to_the_31_floats():
    from isaac_rover_orbit_amd.td3 import FusedTD3, ReplayMemory, TorchTD3
    M, N = 543, 4096                                     # 544 ring slots x 4096 x 965 floats = 8.6 GB
    assert (M + 1) * N * 965 > 2 ** 31
    pol, c1, c2 = nets(13, DEV)
    mem = ReplayMemory(M, N, device=DEV)
    mem.memory_index = mem.cursor = M - 3                 # as if M - 3 adds had happened: the last three fill the last slots
    fill(mem, 3, seed=14)
    assert mem.filled and len(mem) == M * N and mem.ring_pos[-1].item() == M - 1
    g = torch.Generator(device=DEV).manual_seed(3)
    idx = (M - 3) * N + torch.randint(0, 3 * N, (512,), device=DEV, generator=g)
    fused = FusedTD3(pol.state_dict(), c1.state_dict(), c2.state_dict())
    specs = {dt: TorchTD3(*copies((pol, c1, c2), dt)) for dt in (torch.float64, torch.float32)}
    s2 = mem.gather(idx)[3]
    assert float(s2.abs().sum()) > 0                      # the next states live in ring slot 543, past 2^31 floats
    both_steps(mem, fused, specs, idx)


def test_out_of_range_index_is_flagged():
    mem, fused, _ = setup(seed=15, M=4, N=64, steps=2)
    idx = torch.tensor([0, len(mem)], dtype=torch.int64, device=DEV)
    fused.critic_step(mem, idx)
    assert fused.stats()["bad_index"] == 1


def test_two_runs_are_bit_identical():
    runs = []
    for _ in range(2):
        mem, fused, _ = setup(seed=16, M=4, N=128, steps=6)
        g = torch.Generator(device=DEV).manual_seed(4)
        for step in range(4):
            idx = mem.sample_indices(1000, g)
            fused.update(mem, idx, torch.randn(1000, 2, device=DEV, generator=g) if step == 1 else None)
        runs.append((fused.params.clone(), fused.target.clone(), fused.adam_m.clone(), fused.adam_v.clone(), fused.state.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_state_dict_loads_into_the_torch_modules():
    from isaac_rover_orbit_amd.td3 import CHECKPOINT_KEYS, Critic, FusedTD3
    from ppo_reference import load_example
    mem, fused, _ = setup(seed=17, M=4, N=64, steps=5)
    g = torch.Generator(device=DEV).manual_seed(5)
    for _ in range(4):
        fused.update(mem, mem.sample_indices(256, g))
    ck = fused.state_dict()
    assert tuple(ck) == CHECKPOINT_KEYS
    ex = load_example()
    pol, tpol = ex.Net(2, False).to(DEV), ex.Net(2, False).to(DEV)
    pol.load_state_dict(ck["policy"])
    tpol.load_state_dict(ck["target_policy"])
    crit = {k: Critic().to(DEV) for k in ("critic_1", "critic_2", "target_critic_1", "target_critic_2")}
    for k, m in crit.items():
        m.load_state_dict(ck[k])
    s = mem.gather(mem.sample_indices(200, g))[0]
    with torch.no_grad():
        torch.testing.assert_close(fused.actor(s), pol(s), rtol=1e-4, atol=1e-5)
    # a trainer restored from the checkpoint holds the same vectors, and its next y is the loaded target modules' y
    back = FusedTD3.from_checkpoint(ck)
    for name in ("params", "target"):
        assert torch.equal(getattr(back, name), getattr(fused, name))
    gidx = mem.sample_indices(200, g)
    s, a, r, s2, t = mem.gather(gidx)
    with torch.no_grad():
        a2 = tpol(s2)
        y = r + 0.99 * t.logical_not() * torch.min(crit["target_critic_1"](s2, a2), crit["target_critic_2"](s2, a2))
    yk = torch.empty(200, device=DEV)
    back.critic_step(mem, gidx, y_out=yk)
    torch.testing.assert_close(yk, y.reshape(-1), rtol=1e-4, atol=1e-5)
