"""Fused DAgger at 160 x 90 (include/rover_dagger_conv.h) on the MI355X against its specification (isaac_rover_orbit_amd/dagger_conv.py).

The x images, the env columns, the teacher's rows, labels, student actions and indices are compared bit for bit.  The stem's features
and everything the update forms follow td3_helpers.check with its defaults, the rule the TD3, SAC and DAgger updates already meet:
the fused error against the float64 spec stays within that helper's multiple of torch float32's own error (conv2d on the CPU) on the
same inputs.  Loss and norm take ``rel=1e-3``, as in test_gpu_dagger.py.  The specs run on the CPU on copies of the two rings."""
import contextlib
import copy
import ctypes as C
import signal

import numpy as np
import pytest
import torch

from td3_helpers import check, fill, poison_ws
from test_dagger import env_rows
from test_dagger_conv import Steps, images, stem
from test_gpu_dagger import biteq, net, rover_net, same_trainer

DEV = "cuda"
pytestmark = pytest.mark.gpu
RC = 8                                                          # rover_dagger_conv_chunk_rows(): rows per chunk of the stem backward


def DC():
    from isaac_rover_orbit_amd import dagger_conv
    return dagger_conv


def packed_stem(seed):
    m = stem(seed, torch.float32)
    return m, m.packed().to(DEV)


# ---------------------------------------------------------------------------------------------------------------- rows
def rows_against_the_spec(n, d, e, m, vec):
    """One launch into slot 1 of both rings (a slot of the observation ring is 16-byte aligned only when n is a multiple of 4)."""
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    mem, ring = ReplayMemory(2, n, device=DEV), DC().ImageRing(2, n, DEV)
    mem.obs.fill_(-7.0); ring.x.fill_(-7.0)
    teacher = torch.full((n, 965), -7.0, device=DEV)
    DC().fused_conv_rows(vec, d.to(DEV), e.to(DEV), out=mem.obs[1], image_out=ring.x[1], teacher_rows_out=teacher)
    x = DC().preprocess(d)
    assert biteq(ring.x[1].view(n, 90, 160), x)                                           # the x image: bit for bit
    assert biteq(mem.obs[1, :, :4], DC().sanitise(e[:, :4])) and biteq(teacher, DC().sanitise(e))
    for t in (mem.obs, ring.x):
        assert bool((t[0] == -7.0).all()) and bool((t[2] == -7.0).all())
    got = mem.obs[1, :, 4:].cpu()
    with torch.no_grad():
        ref64, ref32 = copy.deepcopy(m).double()(x.double()), m(x)
    print(f"n={n} features: fused err {float((got.double() - ref64).norm()):.3g}, torch fp32 err {float((ref32.double() - ref64).norm()):.3g}, "
          f"norm {float(ref64.norm()):.3g}")
    check(got, ref64, ref32, what="features")
    assert bool(torch.isfinite(got).all())
    return got


@pytest.mark.parametrize("n", [1, 3, 17])
def test_rows_kernel_against_the_spec(n):
    m, vec = packed_stem(n)
    rows_against_the_spec(n, images(n, n), env_rows(n, n), m, vec)
    # the env's permuted view of the buffer, and without the teacher's rows
    d, e = images(n, n + 1).to(DEV), env_rows(n, n).to(DEV)
    a = DC().fused_conv_rows(vec, d, e)
    assert biteq(DC().fused_conv_rows(vec, d.permute(0, 2, 1), e), a)


@pytest.mark.parametrize("kind", ["clip", "ramp"])
def test_rows_kernel_on_an_all_clip_image_and_a_ramp(kind):
    m, vec = packed_stem(5)
    got = rows_against_the_spec(3, images(3, 0, kind), env_rows(3), m, vec)
    if kind == "clip":                       # every window of rows 1..29 sees the same image: one value; rows 0 and 30 another
        g = got.view(3, 31, 31)
        assert bool((g[:, 1:30] == g[0, 1, 0]).all()) and bool((g[:, 0] == g[0, 0, 0]).all()) and float(g[0, 0, 0]) != float(g[0, 1, 0])


def make_env(n):
    from isaac_rover_orbit_amd import terrain as T
    from isaac_rover_orbit_amd.cfg import RoverEnvCfg
    from isaac_rover_orbit_amd.envs import RoverEnv
    ter = T.make_procedural_terrain((512, 512), seed=21, n_rocks=40)
    ter.make_spawns(2 * n, border_offset=2.0)
    cfg = RoverEnvCfg()
    cfg.scene.num_envs, cfg.sim.device, cfg.terrain.kind, cfg.camera = n, "cuda:0", "custom", DC().student_camera_cfg()
    return cfg, RoverEnv(cfg, terrain=ter)


def test_rows_kernel_on_the_real_camera_of_16_envs():
    _, env = make_env(16)
    obs, _ = env.reset()
    obs, *_ = env.step(torch.zeros(16, 2, device=DEV))
    depth = env.extras["depth"]
    assert tuple(depth.shape) == (16, 160, 90) and not depth.is_contiguous()
    m, vec = packed_stem(6)
    got = rows_against_the_spec(16, depth.cpu(), obs["policy"].cpu(), m, vec)
    assert float(got.std()) > 0.0
    env.close()


# ---------------------------------------------------------------------------------------------------------------- act
def test_act_is_the_policy_forward_on_the_rows_the_kernel_wrote():
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    n = 17
    teacher = rover_net(net(30))
    fused = DC().FusedConvDAgger(net(31).state_dict(), stem=stem(3, torch.float32))
    mem, ring = ReplayMemory(4, n, device=DEV), DC().ImageRing(4, n, DEV)
    col = DC().ConvDAggerCollector(teacher, fused, mem, ring, seed=(5 << 32) | 9, env_id_offset=1000)
    steps = Steps(n, 3, seed=n)
    raw, dep, _, _ = (t.to(DEV) for t in steps.at(0))
    col.begin(raw, dep)
    a_s, src = torch.empty(n, 2, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    seen = 0
    for t, beta in enumerate((0.0, 0.5, 1.0)):
        slot, k = mem.obs[mem.cursor].clone(), mem.memory_index
        assert biteq(slot[:, 4:], DC().fused_conv_rows(fused.stem, dep, raw)[:, 4:])          # the features of this step's image
        a = col.act(beta, student_out=a_s, source_out=src).clone()
        assert biteq(a_s, fused.actor(slot))                                   # rover_policy_forward on the row the rows kernel wrote
        assert biteq(mem.actions[k], teacher(DC().sanitise(raw)))             # the label: the teacher on the sanitised env row
        u = torch.from_numpy(DC().mix_uniforms(col.seed, 1000 + np.arange(n), col.counter - 1) < np.float32(beta)).to(DEV)
        assert torch.equal(src.bool(), u) and biteq(a, torch.where(u.unsqueeze(1), mem.actions[k], a_s))
        if beta == 0.0:
            assert biteq(a, a_s) and int(src.sum()) == 0
        if beta == 1.0:
            assert biteq(a, mem.actions[k]) and int(src.sum()) == n
        seen += int(src.sum()) if beta == 0.5 else 0
        raw, dep, rew, term = (x.to(DEV) for x in steps.at(t + 1))
        idx = col.record(raw, dep, rew, term, 33)
        from isaac_rover_orbit_amd.td3_collect import sample_indices
        assert np.array_equal(idx.cpu().numpy(), sample_indices(col.seed, col.counter - 1, 33, len(mem)))
        assert biteq(mem.rewards[k], rew) and torch.equal(mem.terminated[k], term) and int(mem.ring_pos[k]) == t
        assert biteq(ring.x[mem.cursor].view(n, 90, 160), DC().preprocess(dep))
    assert 0 < seen < n and col.state_dict() == {"seed": (5 << 32) | 9, "counter": 6, "env_id_offset": 1000}
    with pytest.raises(ValueError):
        col.act(-0.1)


# ---------------------------------------------------------------------------------------------------------------- update
def setup(seed=0, M=4, N=8, steps=3, bias=None, **hp):
    """A memory of random rows and labels, an image ring of random x in [0, 1], a FusedConvDAgger and the float64 / float32
    TorchConvDAgger (CPU, on copies of the rings) on the same head and stem; every hyper-parameter goes through float32 first."""
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    hp = {k: float(np.float32(v)) for k, v in hp.items()}
    m, st = net(seed, bias), stem(seed + 1, torch.float32)
    mem, ring = ReplayMemory(M, N, device=DEV), DC().ImageRing(M, N, DEV)
    fill(mem, steps, seed=seed + 1)
    ring.x.copy_(torch.rand(ring.x.shape, generator=torch.Generator().manual_seed(seed + 2)))
    fused = DC().FusedConvDAgger(m.state_dict(), stem=st, **hp)
    specs = {dt: DC().TorchConvDAgger(copy.deepcopy(m).cpu().to(dt), copy.deepcopy(st).to(dt), **hp) for dt in (torch.float64, torch.float32)}
    return mem, ring, fused, specs


def on_cpu(mem, ring):
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    m2, r2 = ReplayMemory(mem.memory_size, mem.num_envs, device="cpu"), DC().ImageRing(ring.memory_size, ring.num_envs, "cpu")
    for k in ("obs", "actions", "rewards", "terminated", "ring_pos"):
        getattr(m2, k).copy_(getattr(mem, k))
    m2.memory_index, m2.filled, m2.cursor = mem.memory_index, mem.filled, mem.cursor
    r2.x.copy_(ring.x)
    return m2, r2


def head_grads(spec):
    return {k: p.grad.detach().clone() for k, p in spec.student.named_parameters() if k != "log_std_parameter"}


def head_params(spec):
    return {k: p.detach().clone() for k, p in spec.student.named_parameters() if k != "log_std_parameter"}


def check_update(mem, ring, fused, specs, idx, steps_before=0):
    n = idx.numel()
    dz, rows, drow = torch.empty(n, 2, device=DEV), torch.empty(n, 965, device=DEV), torch.empty(n, 965, device=DEV)
    fused.update(mem, ring, idx, dz_out=dz, rows_out=rows, drow_out=drow)
    cm, cr = on_cpu(mem, ring)
    out = {dt: sp.update(cm, cr, idx.cpu()) for dt, sp in specs.items()}
    r64, r32 = out[torch.float64], out[torch.float32]
    s64, s32 = specs[torch.float64], specs[torch.float32]
    assert biteq(rows[:, :4], r32["rows"][:, :4])
    check(rows[:, 4:], r64["rows"][:, 4:], r32["rows"][:, 4:], what="features")
    check(dz, r64["dz"], r32["dz"], what="dz")
    assert bool((drow[:, :4] == 0).all()) and bool((drow[:, 964] == 0).all()) and bool((r64["drow"][:, 964] == 0).all())
    check(drow[:, 4:], r64["drow"][:, 4:], r32["drow"][:, 4:], what="dRow")
    check(fused.unstem(fused.grad), {k: p.grad for k, p in s64.stem.named_parameters()}, {k: p.grad for k, p in s32.stem.named_parameters()},
          what="stem grad ")
    check(fused.unvector(fused.grad)["policy"], head_grads(s64), head_grads(s32), what="head grad ")
    check(fused.unstem(fused.params), {k: p.detach() for k, p in s64.stem.named_parameters()},
          {k: p.detach() for k, p in s32.stem.named_parameters()}, what="stem params ")
    check(fused.unvector(fused.params)["policy"], head_params(s64), head_params(s32), what="head params ")
    rep = fused.rep_a.view(fused.n_copies, -1)
    assert all(torch.equal(rep[c], fused.params[:fused.n_a]) for c in range(fused.n_copies))
    st = fused.stats()
    assert st["steps"] == steps_before + 1 and st["bad_index"] == 0
    print(f"n={n} loss fused {st['loss']:.9g} float64 {r64['loss']:.9g}; grad_norm fused {st['grad_norm']:.9g} float64 {r64['grad_norm']:.9g}")
    assert st["loss"] == pytest.approx(r64["loss"], rel=1e-3, abs=1e-6)
    assert st["grad_norm"] == pytest.approx(r64["grad_norm"], rel=1e-3, abs=1e-6)
    return st, dz, rows, drow


def sample(mem, n, seed):
    return mem.sample_indices(n, torch.Generator(device=DEV).manual_seed(seed))


@pytest.mark.parametrize("n", [1, RC - 1, RC, RC + 1, 2 * RC + 4])
def test_update_tracks_the_float64_spec(n):
    from isaac_rover_orbit_amd import _lib
    assert _lib.load().rover_dagger_conv_chunk_rows() == RC
    mem, ring, fused, specs = setup(seed=n % 7)
    st, _, _, drow = check_update(mem, ring, fused, specs, sample(mem, n, n))
    assert st["grad_norm"] > 0 and bool((drow[:, 4:964] != 0).any())
    assert bool((fused.stem_block(fused.grad) != 0).all())                    # every stem parameter received a gradient


def test_update_features_are_the_collectors_bits():
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    n = 5
    fused = DC().FusedConvDAgger(net(32).state_dict(), seed=7)
    mem, ring = ReplayMemory(3, n, device=DEV), DC().ImageRing(3, n, DEV)
    col = DC().ConvDAggerCollector(rover_net(net(33)), fused, mem, ring)
    steps = Steps(n, 2)
    col.begin(*(t.to(DEV) for t in steps.at(0)[:2]))
    for t in range(2):
        col.act(0.5)
        col.record(*(x.to(DEV) for x in steps.at(t + 1)))
    idx = torch.arange(2 * n, device=DEV)
    rows = torch.empty(2 * n, 965, device=DEV)
    fused.update(mem, ring, idx, rows_out=rows)                                # the forward runs under the parameters before the step
    assert biteq(rows, mem.gather(idx)[0]) and fused.stats()["bad_index"] == 0


@pytest.mark.parametrize("clip", [0.0, 1e-3])
def test_grad_norm_clip_on_and_off(clip):
    mem, ring, fused, specs = setup(seed=3, grad_norm_clip=clip, learning_rate=1e-3)
    st, *_ = check_update(mem, ring, fused, specs, sample(mem, 20, 1))
    want = 1.0 if clip == 0.0 else clip / (st["grad_norm"] + 1e-6)
    assert st["grad_norm"] > 1e-3 and st["clip_coef"] == pytest.approx(want, rel=1e-6)
    check_update(mem, ring, fused, specs, sample(mem, 20, 2), steps_before=1)


def test_saturated_head_gives_exactly_zero_stem_gradients():
    mem, ring, fused, specs = setup(seed=4, bias=(20.0, -20.0))
    before = fused.params.clone()
    _, dz, _, drow = check_update(mem, ring, fused, specs, sample(mem, 20, 3))
    assert bool((dz == 0.0).all()) and bool((drow == 0.0).all())
    assert bool((fused.grad == 0.0).all()) and torch.equal(fused.params, before)
    for name in ("params", "grad", "adam_m", "adam_v", "rep_a"):
        assert bool(torch.isfinite(getattr(fused, name)).all()), name


def test_duplicate_indices():
    mem, ring, fused, specs = setup(seed=5)
    idx = sample(mem, 20, 4)
    idx[3:12] = idx[2]
    idx[15:] = idx[14]
    check_update(mem, ring, fused, specs, idx)


@pytest.mark.parametrize("bad", [-1, "len", 2 ** 40])
def test_out_of_range_index_is_flagged_and_reads_row_0(bad):
    """rover_td3.h's rule for both rings: the flag goes up and the row is replaced by row 0, so nothing outside either ring is touched:
    everything but the flag is bit for bit the run with 0 in the bad places."""
    mem, ring, fused, _ = setup(seed=6)
    _, _, clean, _ = setup(seed=6)
    ok = sample(mem, 20, 5)
    idx = ok.clone()
    where = torch.tensor([0, 9, 19], device=DEV)
    idx[where] = len(mem) if bad == "len" else bad
    ok[where] = 0
    outs = [[torch.empty(20, w, device=DEV) for w in (2, 965, 965)] for _ in range(2)]
    fused.update(mem, ring, idx, *outs[0])
    clean.update(mem, ring, ok, *outs[1])
    assert fused.stats()["bad_index"] == 1 and clean.stats()["bad_index"] == 0
    for a, b in zip(*outs):
        assert bool(torch.isfinite(b).all()) and biteq(a, b)
    for name in ("params", "grad", "adam_m", "adam_v", "rep_a"):
        assert biteq(getattr(fused, name), getattr(clean, name)), name
    fused.update(mem, ring, ok)
    assert fused.stats()["bad_index"] == 1                                               # sticky


def test_corrupted_ring_position_is_flagged_and_reads_slot_0():
    mem, ring, fused, _ = setup(seed=6)
    mem2, ring2, clean, _ = setup(seed=6)
    mem.ring_pos[1] = mem.slots                                                          # memory slot 1 points past both rings
    mem2.ring_pos[1] = 0
    idx = sample(mem, 20, 6)
    assert bool(((idx // mem.num_envs) == 1).any())
    fused.update(mem, ring, idx)
    clean.update(mem2, ring2, idx)
    assert fused.stats()["bad_index"] == 1 and clean.stats()["bad_index"] == 0
    for name in ("params", "grad", "adam_m", "adam_v", "rep_a"):
        assert biteq(getattr(fused, name), getattr(clean, name)), name


def test_poisoned_workspace_and_a_smaller_batch():
    mem, ring, fused, _ = setup(seed=7)
    _, _, fresh, _ = setup(seed=7)
    big, small = sample(mem, 24, 6), sample(mem, 11, 7)
    keep = {k: getattr(fused, k).clone() for k in ("params", "adam_m", "adam_v", "state", "rep_a")}
    fused.update(mem, ring, big)
    for k, v in keep.items():                                                            # back to the start; the workspace stays dirty
        getattr(fused, k).copy_(v)
    fused.update(mem, ring, small)
    poison_ws(fresh, 24)                                                                 # every float of the workspace a NaN
    fresh.update(mem, ring, small)
    same_trainer(fused, fresh)
    assert bool(torch.isfinite(fresh.params).all()) and bool(torch.isfinite(fresh.grad).all())


def test_two_runs_are_bit_identical():
    runs = []
    for _ in range(2):
        mem, ring, fused, _ = setup(seed=8)
        for k in range(4):
            fused.update(mem, ring, sample(mem, 21, 7 + k))
        runs.append(fused)
    same_trainer(*runs)
    assert runs[0].stats()["steps"] == 4


# ---------------------------------------------------------------------------------------------------------------- the loop
def loop(n, steps, M=4, seed=11, **hp):
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    teacher = rover_net(net(40))
    fused = DC().FusedConvDAgger(net(41).state_dict(), seed=seed, **hp)
    mem, ring = ReplayMemory(M, n, device=DEV), DC().ImageRing(M, n, DEV)
    col = DC().ConvDAggerCollector(teacher, fused, mem, ring, seed=seed)
    data = Steps(n, steps, seed=seed)
    return teacher, fused, mem, ring, col, [tuple(x.to(DEV) for x in data.at(t)) for t in range(steps + 1)]


def run(fused, col, data, betas, first=0, batch=24, begin=True):
    if begin:
        col.begin(data[first][0], data[first][1])
    acts = []
    for t, beta in enumerate(betas, start=first):
        acts.append(col.act(beta).clone())
        raw, dep, rew, term = data[t + 1]
        fused.update(col.memory, col.images, col.record(raw, dep, rew, term, batch))
    return acts


def test_resume_continues_bit_for_bit():
    betas = [1.0, 0.8, 0.6, 0.4, 0.2]
    teacher, fused, mem, ring, col, data = loop(6, 5)
    acts = run(fused, col, data, betas[:3])
    sd_t, sd_c, mem2, ring2 = fused.state_dict(mem), col.state_dict(), copy.deepcopy(mem), copy.deepcopy(ring)
    assert sd_t["ring"] == {"memory_index": 3, "filled": False, "cursor": 3} and DC().STEM_KEY in sd_t and "policy" in sd_t
    acts += run(fused, col, data, betas[3:], first=3, begin=False)
    again = DC().FusedConvDAgger(net(99).state_dict(), seed=5)
    mem2.memory_index, mem2.cursor = 0, 0
    again.load_state_dict(sd_t, mem2)
    col2 = DC().ConvDAggerCollector(teacher, again, mem2, ring2, seed=0)
    col2.load_state_dict(sd_c)
    col2.resume(data[3][0])                                       # the teacher's rows; the rings keep the slot the last record wrote
    rest = run(again, col2, data, betas[3:], first=3, begin=False)
    assert all(biteq(x, y) for x, y in zip(acts[3:], rest))
    same_trainer(fused, again)
    assert biteq(mem.obs, mem2.obs) and biteq(mem.actions, mem2.actions) and biteq(ring.x, ring2.x)
    # the checkpoint: the head as FusedDAgger writes it (RoverNet loads it), the stem as ConvStem's state_dict
    ck = fused.checkpoint()
    student = DC().ConvStudent.from_checkpoint(ck)
    raw, dep = data[5][0], data[5][1]
    assert biteq(student.act(raw, dep), fused.actor(DC().fused_conv_rows(fused.stem, dep, raw)))
    assert biteq(DC().ConvStem.from_packed(fused.stem.cpu()).packed(), fused.stem)


def test_act_record_update_do_not_synchronise():
    teacher, fused, mem, ring, col, data = loop(8, 4)
    run(fused, col, data, [0.5])                                   # every buffer is allocated, every kernel has run once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        run(fused, col, data, [0.9, 0.5, 0.1], first=1, begin=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    st = fused.stats()
    assert st["steps"] == 4 and st["bad_index"] == 0 and np.isfinite(st["loss"])


@contextlib.contextmanager
def time_limit(seconds):
    """Ends the block with a TimeoutError after ``seconds`` (SIGALRM: the suite runs its tests on the main thread)."""
    def stop(signum, frame):
        raise TimeoutError(f"no result after {seconds} s")
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def test_end_to_end_16_envs_20_steps_in_a_4_slot_memory():
    with time_limit(120):
        end_to_end()


def end_to_end():
    """The example's loop on the real env and its 160 x 90 camera: beta from 1 down to 0, one update per step, the memory wraps four
    times; no claim about how well the student drives."""
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    n, steps = 16, 20
    cfg, env = make_env(n)
    fused = DC().FusedConvDAgger(net(51).state_dict(), seed=3)
    before = fused.stem.clone()
    mem, ring = ReplayMemory(4, n, device=DEV), DC().ImageRing(4, n, DEV)
    col = DC().ConvDAggerCollector(rover_net(net(50)), fused, mem, ring, seed=3, env_id_offset=cfg.env_id_offset)
    obs, _ = env.reset()
    col.begin(obs, env.extras["depth"])
    losses = torch.empty(steps, device=DEV)
    for t in range(steps):
        obs, rew, term, trunc, _ = env.step(col.act(1.0 - t / (steps - 1)))
        fused.update(mem, ring, col.record(obs, env.extras["depth"], rew, term, 32))
        losses[t] = fused.state.view(torch.float32)[2]             # rover_dagger_state.loss, copied on the device
    st = fused.stats()
    assert bool(torch.isfinite(losses).all()) and st["bad_index"] == 0 and st["steps"] == steps and mem.filled
    assert bool(torch.isfinite(fused.params).all()) and not torch.equal(fused.stem, before)
    assert float(ring.x.min()) >= 0.0 and float(ring.x.max()) <= 1.0 and float(ring.x.std()) > 0.0
    student = DC().ConvStudent.from_checkpoint(fused.checkpoint())
    assert biteq(student.act(obs, env.extras["depth"]), fused.actor(DC().fused_conv_rows(fused.stem, env.extras["depth"], obs["policy"])))
    env.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_return_codes_not_faults():
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd.dagger import default_hparams
    lib = _lib.load()
    mem, ring, fused, _ = setup(seed=9)
    idx = sample(mem, 8, 1)
    fused._ensure_ws(8)
    before = fused.params.clone()

    def update(**kw):
        a = dict(desc=C.byref(fused.desc_a), hp=C.byref(fused.hp), params=fused.params.data_ptr(), grad=fused.grad.data_ptr(),
                 m=fused.adam_m.data_ptr(), v=fused.adam_v.data_ptr(), obs=mem.obs.data_ptr(), img=ring.x.data_ptr(), img_slots=ring.slots,
                 h=90, w=160, slots=mem.slots, envs=mem.num_envs, pos=mem.ring_pos.data_ptr(), labels=mem.actions.data_ptr(),
                 idx=idx.data_ptr(), n=8, valid=len(mem), ws=fused.ws.data_ptr(), ws_bytes=fused.ws.numel(), state=fused.state.data_ptr(),
                 rep=fused.rep_a.data_ptr(), copies=fused.n_copies, dz=None, rows=None, drow=None, stream=None)
        a.update(kw)
        return lib.rover_dagger_conv_update(*a.values())

    INVALID, UNSUPPORTED = 1, 4
    assert update(h=31, w=31) == UNSUPPORTED and b"90 x 160" in lib.rover_last_error()
    assert update(h=160, w=90) == UNSUPPORTED
    for name in ("hp", "params", "grad", "m", "v", "obs", "img", "pos", "labels", "idx", "ws", "state", "desc"):
        assert update(**{name: None}) == INVALID, name
    assert update(n=0) == INVALID and update(n=-3) == INVALID
    assert update(img_slots=mem.slots - 1) == INVALID and b"image ring" in lib.rover_last_error()
    assert update(ws_bytes=fused.ws.numel() // 2) == INVALID
    assert update(img=ring.x.data_ptr() + 4) == INVALID                                    # the images are read 16 bytes at a time
    # the rows entry
    vec, d, e = fused.stem, torch.zeros(2, 14400, device=DEV), torch.zeros(2, 965, device=DEV)
    out, x = torch.zeros(2, 965, device=DEV), torch.zeros(2, 14400, device=DEV)
    hp = default_hparams()

    def rows(**kw):
        a = dict(hp=C.byref(hp), stem=vec.data_ptr(), depth=d.data_ptr(), h=90, w=160, env=e.data_ptr(), n=2, out=out.data_ptr(),
                 x=x.data_ptr(), teacher=None, rew=None, term=None, rew_out=None, term_out=None, pos=None, pos_value=0, idx=None, batch=0,
                 mem_rows=0, counter=C.c_uint64(0), stream=None)
        a.update(kw)
        return lib.rover_dagger_conv_rows(*a.values())

    assert rows(h=31, w=31) == UNSUPPORTED and rows(h=90, w=161) == UNSUPPORTED
    for name in ("hp", "stem", "depth", "env", "out", "x"):
        assert rows(**{name: None}) == INVALID, name
    assert rows(n=0) == INVALID and rows(out=e.data_ptr()) == INVALID and rows(depth=d.data_ptr() + 4) == INVALID
    assert rows(idx=idx.data_ptr(), batch=0, mem_rows=10) == INVALID and rows(idx=idx.data_ptr(), batch=8, mem_rows=0) == INVALID
    assert rows(rew=e.data_ptr()) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(fused.params, before) and fused.stats()["steps"] == 0               # nothing was launched
    assert rows() == 0 and update() == 0
    # and through the Python layer
    with pytest.raises(_lib.RoverHipError):
        fused.update(mem, ring, idx, img_h=31, img_w=31)
    with pytest.raises(ValueError):
        DC().fused_conv_rows(vec, torch.zeros(2, 31, 31, device=DEV), e)
    with pytest.raises(ValueError):
        DC().ConvDAggerCollector(rover_net(net(1)), fused, mem, DC().ImageRing(mem.memory_size - 1, mem.num_envs, DEV))
