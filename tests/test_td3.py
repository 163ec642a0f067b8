"""TD3, CPU side: the replay memory's ring against skrl's two-buffer RandomMemory, the torch spec's policy delay, target copies,
Polyak formula and bootstrap rule, and the host-only parts of include/rover_td3.h."""
import ctypes as C

import pytest
import torch

from td3_helpers import fill, nets


# ---- replay memory
@pytest.mark.parametrize("M,steps", [(1, 1), (1, 4), (3, 2), (3, 3), (3, 11), (5, 17)])
@pytest.mark.parametrize("identity", [True, False])
def test_ring_memory_matches_two_buffer_memory(M, steps, identity):
    from doubles.skrl.memories.torch import RandomMemory
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    N, D = 4, 7
    mem = ReplayMemory(M, N, device="cpu", obs_dim=D)
    ref = RandomMemory(memory_size=M, num_envs=N, device="cpu")
    for name, size, dt in (("states", D, torch.float32), ("actions", 2, torch.float32), ("rewards", 1, torch.float32),
                           ("next_states", D, torch.float32), ("terminated", 1, torch.bool)):
        ref.create_tensor(name, size, dt)
    g = torch.Generator().manual_seed(5)
    states = torch.randn(N, D, generator=g)
    for t in range(steps):
        actions, rewards = torch.randn(N, 2, generator=g), torch.randn(N, 1, generator=g)
        next_states, terminated = torch.randn(N, D, generator=g), torch.rand(N, 1, generator=g) < 0.3
        mem.add(states, actions, rewards, next_states, terminated)
        ref.add_samples(states=states, actions=actions, rewards=rewards, next_states=next_states, terminated=terminated)
        assert len(mem) == len(ref) == min(t + 1, M) * N
        # every filled row, plus a random draw with replacement
        idx = torch.cat([torch.arange(len(mem)), mem.sample_indices(64, g)])
        got = mem.gather(idx)
        for x, name in zip(got, ("states", "actions", "rewards", "next_states", "terminated")):
            want = ref.get_tensor_by_name(name, keepdim=False)[idx]
            assert x.dtype == want.dtype and torch.equal(x, want), (t, name)
        if identity:
            states = next_states
        else:
            states = states.clone()
            states.copy_(next_states)


def test_memory_length_counts_filled_slots_and_sizes():
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    mem = ReplayMemory(4, 3, device="cpu", obs_dim=5)
    assert len(mem) == 0
    with pytest.raises(ValueError):
        mem.sample_indices(2)
    fill(mem, 2)
    assert len(mem) == 6
    idx = mem.sample_indices(1000, torch.Generator().manual_seed(0))
    assert int(idx.min()) >= 0 and int(idx.max()) < 6
    fill(mem, 9)
    assert len(mem) == 12
    # the reference's size: 8192 slots x 4096 envs x 965 floats: one ring is half of skrl's two buffers (259 GB -> 129.5 GB)
    assert ReplayMemory.nbytes(8192, 4096) < 0.51 * ReplayMemory.two_buffer_nbytes(8192, 4096)
    assert abs(4 * 8193 * 4096 * 965 / 1e9 - 129.5) < 0.1


# ---- torch spec
def _spec(seed=0, dtype=torch.float64, **hp):
    from isaac_rover_orbit_amd.td3 import TorchTD3
    pol, c1, c2 = (m.to(dtype) for m in nets(seed))
    return TorchTD3(pol, c1, c2, **hp)


def _memory(M=3, N=8, steps=5):
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    mem = ReplayMemory(M, N, device="cpu")
    fill(mem, steps)
    return mem


def _flat(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()])


def test_targets_start_as_copies():
    spec = _spec()
    for t, m in ((spec.target_policy, spec.policy), (spec.target_critic_1, spec.critic_1), (spec.target_critic_2, spec.critic_2)):
        assert t is not m and torch.equal(_flat(t), _flat(m))


@pytest.mark.parametrize("delay", [1, 2, 3])
def test_actor_steps_only_on_every_policy_delay_th_critic_step(delay):
    spec = _spec(policy_delay=delay)
    mem = _memory()
    g = torch.Generator().manual_seed(3)
    for step in range(1, 7):
        before = {k: _flat(getattr(spec, k)) for k in ("policy", "target_policy", "critic_1", "target_critic_1")}
        st = spec.update(mem, mem.sample_indices(16, g))
        stepped = step % delay == 0
        assert st["actor_stepped"] == stepped
        assert not torch.equal(_flat(spec.critic_1), before["critic_1"])
        for k in ("policy", "target_policy", "target_critic_1"):
            assert torch.equal(_flat(getattr(spec, k)), before[k]) != stepped, (step, k)
    assert spec.critic_update_counter == 6


def test_polyak_is_skrls_update_parameters_formula():
    from isaac_rover_orbit_amd.td3 import update_parameters
    pol = nets(1)[0]
    tgt = nets(2)[0]
    t0, p0 = _flat(tgt), _flat(pol)
    update_parameters(tgt, pol, 0.005)
    want = t0.clone()
    want.mul_(1 - 0.005)
    want.add_(0.005 * p0)
    assert torch.equal(_flat(tgt), want)
    # fp32 rounding: two products and one sum, not a fused or reordered form
    assert torch.equal(want, (t0 * torch.tensor(0.995, dtype=torch.float32)) + (p0 * torch.tensor(0.005, dtype=torch.float32)))
    update_parameters(tgt, pol, 1)
    assert torch.equal(_flat(tgt), p0)


def test_terminated_rows_get_reward_and_truncated_rows_bootstrap():
    spec = _spec(dtype=torch.float32)
    g = torch.Generator().manual_seed(4)
    B = 32
    s2 = torch.randn(B, 965, generator=g) * 0.5
    r = torch.randn(B, 1, generator=g)
    term = (torch.arange(B) % 3 == 0).unsqueeze(1)
    y = spec.target_values(s2, r, term)
    assert torch.equal(y[term], r[term])
    with torch.no_grad():
        a2 = spec.target_policy(s2)
        q = torch.min(spec.target_critic_1(s2, a2), spec.target_critic_2(s2, a2))
    live = ~term
    assert torch.equal(y[live], (r + 0.99 * q)[live])
    assert not torch.equal(y[live], r[live])


def test_smoothing_noise_is_clipped_then_the_action_clamped():
    spec = _spec()
    g = torch.Generator().manual_seed(6)
    B = 16
    s2 = torch.randn(B, 965, generator=g, dtype=torch.float64) * 0.5
    r = torch.zeros(B, 1, dtype=torch.float64)
    term = torch.zeros(B, 1, dtype=torch.bool)
    noise = torch.randn(B, 2, generator=g, dtype=torch.float64) * 3
    y = spec.target_values(s2, r, term, noise)
    with torch.no_grad():
        a2 = (spec.target_policy(s2) + noise.clamp(-0.5, 0.5)).clamp(-1, 1)
        want = 0.99 * torch.min(spec.target_critic_1(s2, a2), spec.target_critic_2(s2, a2))
    # gamma * !terminated is a float32 tensor (skrl's expression), so gamma enters a float64 spec as (float)0.99
    assert torch.allclose(y, want, rtol=1e-7, atol=0)


def test_exploration_schedule_is_linear_then_off():
    from isaac_rover_orbit_amd.td3 import exploration_scale, explore
    assert exploration_scale(0, 100) == 1.0
    assert exploration_scale(50, 100) == pytest.approx(0.5 * (1 - 1e-3) + 1e-3)
    assert exploration_scale(100, 100) == pytest.approx(1e-3)
    assert exploration_scale(101, 100) is None
    a = torch.tensor([[0.9, -0.2]])
    assert torch.equal(explore(a, torch.ones(1, 2), None), a)
    assert torch.equal(explore(a, torch.ones(1, 2), 0.5), torch.tensor([[1.0, 0.3]]))


# ---- host-only ABI checks
def _descs():
    from isaac_rover_orbit_amd import td3
    from isaac_rover_orbit_amd.ppo import pack
    pol, c1, _ = nets(0)
    da, _ = pack(pol.state_dict(), "none")
    dc, _ = td3.pack_critic(c1.state_dict())
    return da, dc


def test_struct_mirrors_and_sizes():
    from isaac_rover_orbit_amd import _lib, build
    from isaac_rover_orbit_amd.td3 import HPARAMS, default_hparams
    build.build_extension()
    lib = _lib.load()
    assert lib.rover_td3_hparams_bytes() == C.sizeof(_lib.Td3Hparams) == 40
    assert lib.rover_td3_state_bytes() == C.sizeof(_lib.Td3State) == 64
    h = default_hparams()
    want = dict(gamma=HPARAMS["discount_factor"], polyak=HPARAMS["polyak"], actor_lr=HPARAMS["actor_learning_rate"],
                critic_lr=HPARAMS["critic_learning_rate"], beta1=0.9, beta2=0.999, eps=1e-8,
                noise_clip=HPARAMS["smooth_regularization_clip"], act_min=-1.0, act_max=1.0)
    for k, v in want.items():
        assert getattr(h, k) == pytest.approx(v, rel=1e-7), k
    da, dc = _descs()
    na, nc = lib.rover_policy_packed_floats(C.byref(da)), lib.rover_policy_packed_floats(C.byref(dc))
    P = lib.rover_td3_param_floats(C.byref(da), C.byref(dc))
    assert P == (na + 2 * nc + 63) // 64 * 64
    assert lib.rover_td3_param_floats(C.byref(dc), C.byref(da)) == 0
    assert lib.rover_td3_workspace_bytes(0) == 0 and lib.rover_td3_workspace_bytes(1) > 0
    assert lib.rover_td3_workspace_bytes(4097) > lib.rover_td3_workspace_bytes(4096)


def test_critic_pack_reads_back_through_policy_unpack():
    from isaac_rover_orbit_amd import build, td3
    from isaac_rover_orbit_amd.ppo import unpack
    build.build_extension()
    _, c1, _ = nets(3)
    sd = c1.state_dict()
    desc, packed = td3.pack_critic(sd)
    assert desc.layers[2].K == 66 and desc.layers[5].N == 1
    back = unpack(desc, torch.from_numpy(packed))
    assert set(back) == set(sd)
    for k, v in sd.items():
        assert torch.equal(back[k], v), k
    fresh = td3.Critic()
    fresh.load_state_dict(back)


def test_bad_arguments_return_error_codes():
    from isaac_rover_orbit_amd import _lib, build
    from isaac_rover_orbit_amd.td3 import critic_desc, default_hparams
    build.build_extension()
    lib = _lib.load()
    da, dc = _descs()
    h = default_hparams()
    fake = C.c_void_p(1 << 20)        # aligned, never dereferenced: every check below fails before any device access

    def critic_step(a=da, c=dc, hh=h, params=fake, ws=fake, ws_bytes=1 << 40, n=16, slots=3, envs=8, valid=16, idx=fake):
        return lib.rover_td3_critic_step(C.byref(a) if a is not None else None, C.byref(c) if c is not None else None,
                                         C.byref(hh) if hh is not None else None, params, fake, fake, fake, fake, fake, slots, envs,
                                         fake, fake, fake, fake, idx, n, valid, None, ws, ws_bytes, fake, None, None)

    def actor_step(a=da, c=dc, params=fake, ws_bytes=1 << 40, n=16):
        return lib.rover_td3_actor_step(C.byref(a), C.byref(c), C.byref(h), params, fake, fake, fake, fake, 3, 8, fake, fake, n, 16,
                                        fake, ws_bytes, fake, None, 1, None, None)
    assert critic_step(a=None) == 1 and critic_step(c=None) == 1
    assert critic_step(hh=None) == 1 and critic_step(params=None) == 1 and critic_step(idx=None) == 1
    assert actor_step(params=None) == 1
    assert critic_step(n=0) == 1 and critic_step(slots=1) == 1 and critic_step(valid=17) == 1
    small = lib.rover_td3_workspace_bytes(16) - 1
    assert critic_step(ws_bytes=small) == 1 and b"workspace too small" in lib.rover_last_error()
    assert actor_step(ws_bytes=small) == 1
    # non-TD3 descriptors: the lift network, the PPO policy (final tanh), the unpacked critic layout, swapped roles
    lift = _lib.PolicyDesc()
    lib.rover_lift_policy_desc(C.byref(lift), 8)
    tanh = _lib.PolicyDesc.from_buffer_copy(da)
    tanh.layers[5].act = _lib.ACT_TANH
    for a, c in ((lift, dc), (tanh, dc), (da, critic_desc()), (dc, da), (da, lift)):
        assert critic_step(a=a, c=c) == 4
        assert b"TD3" in lib.rover_last_error()
        assert actor_step(a=a, c=c) == 4
    assert lib.rover_td3_polyak(None, fake, fake, 4, None) == 1 and lib.rover_td3_polyak(C.byref(h), None, fake, 4, None) == 1
    assert lib.rover_td3_critic_desc(None) == 1
    # the critic pack refuses other layouts; rover_policy_pack and rover_policy_forward refuse the critic
    import numpy as np
    w = [np.zeros((dc.layers[i].N, dc.layers[i].K), np.float32) for i in range(6)]
    b = [np.zeros(dc.layers[i].N, np.float32) for i in range(6)]
    wp = (C.c_void_p * 6)(*[x.ctypes.data for x in w])
    bp = (C.c_void_p * 6)(*[x.ctypes.data for x in b])
    out = np.zeros(lib.rover_policy_packed_floats(C.byref(dc)), np.float32)
    assert lib.rover_td3_critic_pack(C.byref(_lib.PolicyDesc.from_buffer_copy(da)), wp, bp, out.ctypes.data) == 4
    assert lib.rover_policy_pack(C.byref(_lib.PolicyDesc.from_buffer_copy(dc)), wp, bp, out.ctypes.data) != 0
    assert lib.rover_policy_forward(C.byref(dc), fake, 1, fake, 16, fake, None) != 0
    assert b"chain" in lib.rover_last_error()
