"""Fused DAgger (include/rover_dagger.h) on the MI355X against its specification (isaac_rover_orbit_amd/dagger.py).

Rows, labels, student actions, sources and indices are compared bit for bit.  The update follows td3_helpers.check, the rule
test_gpu_td3_update.py uses for the same network kernels: the fused error against the float64 spec stays within that helper's multiple
of torch fp32's own error on the same inputs; the loss in the state block takes the bound the TD3 test puts on its losses."""
import contextlib
import copy
import os
import signal
import tempfile

import numpy as np
import pytest
import torch

from ppo_reference import load_example
from td3_helpers import check, fill, poison_ws
from test_dagger import Steps, env_rows, images

DEV = "cuda"
pytestmark = pytest.mark.gpu
CH = 512                                                        # offpolicy_net.hpp: rows per weight-gradient chunk


def D():
    from isaac_rover_orbit_amd import dagger
    return dagger


def biteq(a, b):
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def net(seed, bias=None):
    torch.manual_seed(seed)
    m = load_example().Net(2, True).to(DEV)
    if bias is not None:
        with torch.no_grad():
            m.mlp[6].bias.copy_(torch.tensor(bias))
    return m


def rover_net(module):
    from isaac_rover_orbit_amd.policy import RoverNet
    return RoverNet.from_state_dict(module.state_dict(), final_act="tanh")


# ---------------------------------------------------------------------------------------------------------------- rows
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_rows_kernel_is_bit_equal_to_the_spec(n):
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    d, e = images(n, n).to(DEV), env_rows(n, n).to(DEV)
    d.view(n, -1)[:, 5] = 2 * 10.0
    e[0, :4] = torch.tensor([float("nan"), float("inf"), -float("inf"), 1.5], device=DEV)
    want = D().student_rows(d.cpu(), e.cpu())
    teacher = torch.empty(n, 965, device=DEV)
    got = D().fused_student_rows(d, e, teacher_rows_out=teacher)              # fresh allocations: the 16-byte path
    assert biteq(got, want) and biteq(teacher, D().sanitise(e.cpu()))
    assert biteq(D().fused_student_rows(d, e), want)                           # without the teacher's rows
    assert biteq(D().fused_student_rows(d.permute(0, 2, 1), e), want)          # the env's permuted view of the buffer
    # into ring slot 1, which is 16-byte aligned only when n is a multiple of 4, and from an image that never is: float by float
    mem = ReplayMemory(2, n, device=DEV)
    mem.obs.fill_(-7.0)
    D().fused_student_rows(d, e, out=mem.obs[1])
    pad = torch.zeros(n * 961 + 1, device=DEV)
    pad[1:] = d.reshape(-1)
    assert biteq(mem.obs[1], want) and bool((mem.obs[0] == -7.0).all()) and bool((mem.obs[2] == -7.0).all())
    assert biteq(D().fused_student_rows(pad[1:].view(n, 961), e), want)
    # other hyper-parameters
    assert biteq(D().fused_student_rows(d, e, depth_clip=5.0, depth_scale=2.0), D().student_rows(d.cpu(), e.cpu(), 5.0, 2.0))


def test_rows_kernel_on_the_real_camera_of_64_envs():
    from isaac_rover_orbit_amd import terrain as T
    from isaac_rover_orbit_amd.cfg import RoverEnvCfg
    from isaac_rover_orbit_amd.envs import RoverEnv
    ter = T.make_procedural_terrain((512, 512), seed=21, n_rocks=40)
    ter.make_spawns(2 * 64, border_offset=2.0)
    cfg = RoverEnvCfg()
    cfg.scene.num_envs, cfg.sim.device, cfg.terrain.kind, cfg.camera = 64, "cuda:0", "custom", D().student_camera_cfg()
    env = RoverEnv(cfg, terrain=ter)
    obs, _ = env.reset()
    obs, *_ = env.step(torch.zeros(64, 2, device=DEV))
    depth = env.extras["depth"]
    assert tuple(depth.shape) == (64, 31, 31) and not depth.is_contiguous()
    got = D().fused_student_rows(depth, obs["policy"])
    want = D().student_rows(depth.cpu(), obs["policy"].cpu())
    assert biteq(got, want) and bool(torch.isfinite(got).all())
    assert float(got[:, 4:].min()) >= 0.0 and float(got[:, 4:].max()) <= 1.0 and float(got[:, 4:].std()) > 0.0
    env.close()


# ---------------------------------------------------------------------------------------------------------------- act
@pytest.mark.parametrize("n", [1, 17, 257])
def test_act_labels_student_and_mix(n):
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    teacher, student = rover_net(net(30)), rover_net(net(31))
    steps = Steps(n, 3, seed=n)
    mem, ref = ReplayMemory(4, n, device=DEV), ReplayMemory(4, n, device="cpu")
    col = D().DAggerCollector(teacher, student, mem, seed=(5 << 32) | 9, env_id_offset=1000)
    a_s, src = torch.empty(n, 2, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    # the spec runs on the CPU with the fused networks as its callables: only the draw, the mix and the bookkeeping are its own
    spec = D().TorchDAggerCollector(lambda r: teacher(r.to(DEV)).cpu(), lambda r: student(r.to(DEV)).cpu(), ref, seed=(5 << 32) | 9,
                                    env_id_offset=1000)
    raw, dep, _, _ = steps.at(0)
    col.begin(raw.to(DEV), dep.to(DEV)); spec.begin(raw, dep)
    seen = 0
    for t, beta in enumerate((0.0, 0.5, 1.0)):
        slot, k = mem.obs[mem.cursor].clone(), mem.memory_index
        assert col.counter == spec.counter
        a = col.act(beta, student_out=a_s, source_out=src).clone()
        want = spec.act(beta)
        assert biteq(a_s, student(slot))                                       # the student forward: rover_policy_forward on the slot
        assert biteq(mem.actions[k], teacher(D().sanitise(raw.to(DEV))))       # the label: the teacher on the sanitised env row
        assert torch.equal(src.cpu().bool(), spec.last["source"]) and biteq(a, want)
        assert biteq(mem.actions[k], spec.last["label"]) and biteq(a_s, spec.last["student"])
        assert int(src.sum()) == {0.0: 0, 1.0: n}.get(beta, int(src.sum()))
        seen += int(src.sum()) if beta == 0.5 else 0
        raw, dep, rew, term = steps.at(t + 1)
        idx = col.record(raw.to(DEV), dep.to(DEV), rew.to(DEV), term.to(DEV), 33)
        assert torch.equal(idx.cpu(), spec.record(raw, dep, rew, term, 33))
        assert biteq(mem.obs, ref.obs) and biteq(mem.rewards, ref.rewards) and torch.equal(mem.terminated.cpu(), ref.terminated)
        assert torch.equal(mem.ring_pos.cpu(), ref.ring_pos)
        assert (mem.memory_index, mem.cursor, len(mem)) == (ref.memory_index, ref.cursor, len(ref))
    assert col.state_dict() == spec.state_dict() == {"seed": (5 << 32) | 9, "counter": 6, "env_id_offset": 1000}
    assert n < 17 or 0 < seen < n
    with pytest.raises(ValueError):
        col.act(-0.1)


# ---------------------------------------------------------------------------------------------------------------- update
def setup(seed=0, M=4, N=64, steps=6, bias=None, **hp):
    """A memory of random rows and labels in [-1, 1], a FusedDAgger and the float64 / float32 TorchDAgger on the same student; every
    hyper-parameter goes through float32 first, so both paths hold the number the C struct holds."""
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    hp = {k: float(np.float32(v)) for k, v in hp.items()}
    m = net(seed, bias)
    mem = ReplayMemory(M, N, device=DEV)
    fill(mem, steps, seed=seed + 1)
    fused = D().FusedDAgger(m.state_dict(), **hp)
    specs = {dt: D().TorchDAgger(copy.deepcopy(m).to(dt), **hp) for dt in (torch.float64, torch.float32)}
    return mem, fused, specs


def grads(spec):
    return {k: p.grad.detach().clone() for k, p in spec.student.named_parameters() if k != "log_std_parameter"}


def params(spec):
    return {k: p.detach().clone() for k, p in spec.student.named_parameters() if k != "log_std_parameter"}


def check_update(mem, fused, specs, idx, steps_before=0):
    dz = torch.empty(idx.numel(), 2, device=DEV)
    fused.update(mem, idx, dz_out=dz)
    out = {dt: sp.update(mem, idx) for dt, sp in specs.items()}
    r64, r32 = out[torch.float64], out[torch.float32]
    check(dz, r64["dz"], r32["dz"], what="dz")
    check(fused.unvector(fused.grad)["policy"], grads(specs[torch.float64]), grads(specs[torch.float32]), what="grad ")
    check(fused.unvector(fused.params)["policy"], params(specs[torch.float64]), params(specs[torch.float32]), what="params ")
    rep = fused.rep_a.view(fused.n_copies, -1)
    assert all(torch.equal(rep[c], fused.params[:fused.n_a]) for c in range(fused.n_copies))
    st = fused.stats()
    assert st["steps"] == steps_before + 1 and st["bad_index"] == 0
    print(f"n={idx.numel()} loss fused {st['loss']:.9g} float64 {r64['loss']:.9g}; grad_norm fused {st['grad_norm']:.9g} float64 "
          f"{r64['grad_norm']:.9g}")
    assert st["loss"] == pytest.approx(r64["loss"], rel=1e-3, abs=1e-6)
    assert st["grad_norm"] == pytest.approx(r64["grad_norm"], rel=1e-3, abs=1e-6)
    return st, dz


@pytest.mark.parametrize("n", [1, 15, 16, 17, CH - 1, CH, CH + 1])
def test_update_tracks_the_float64_spec(n):
    mem, fused, specs = setup(seed=n % 7, M=4, N=160, steps=5)
    check_update(mem, fused, specs, mem.sample_indices(n, torch.Generator(device=DEV).manual_seed(n)))


@pytest.mark.parametrize("clip", [0.0, 1e-3])
def test_grad_norm_clip_on_and_off(clip):
    mem, fused, specs = setup(seed=3, grad_norm_clip=clip, learning_rate=1e-3)
    st, _ = check_update(mem, fused, specs, mem.sample_indices(300, torch.Generator(device=DEV).manual_seed(1)))
    want = 1.0 if clip == 0.0 else clip / (st["grad_norm"] + 1e-6)
    assert st["grad_norm"] > 1e-3 and st["clip_coef"] == pytest.approx(want, rel=1e-6)
    check_update(mem, fused, specs, mem.sample_indices(300, torch.Generator(device=DEV).manual_seed(2)), steps_before=1)


def test_saturated_outputs_give_exactly_zero_dz_and_no_nan():
    mem, fused, specs = setup(seed=4, bias=(20.0, -20.0))
    idx = mem.sample_indices(200, torch.Generator(device=DEV).manual_seed(3))
    rows = mem.gather(idx)[0]
    out = fused.actor(rows)
    assert bool((out[:, 0] == 1.0).all()) and bool((out[:, 1] == -1.0).all())           # |tanh z| = 1 in fp32
    before = fused.params.clone()
    _, dz = check_update(mem, fused, specs, idx)
    assert bool((dz == 0.0).all())
    for name in ("params", "grad", "adam_m", "adam_v", "rep_a"):
        assert bool(torch.isfinite(getattr(fused, name)).all()), name
    assert bool((fused.grad == 0.0).all()) and torch.equal(fused.params, before)


def test_duplicate_indices():
    mem, fused, specs = setup(seed=5)
    idx = mem.sample_indices(64, torch.Generator(device=DEV).manual_seed(4))
    idx[10:40] = idx[3]
    idx[50:] = idx[49]
    check_update(mem, fused, specs, idx)


@pytest.mark.parametrize("bad", [-1, "len", 2 ** 40])
def test_out_of_range_index_is_flagged_and_reads_row_0(bad):
    """rover_td3.h's rule: the flag goes up and the row is replaced by row 0, so nothing outside the memory is touched: everything
    but the flag is bit for bit the run with 0 in the bad places."""
    mem, fused, _ = setup(seed=6)
    _, clean, _ = setup(seed=6)
    ok = mem.sample_indices(300, torch.Generator(device=DEV).manual_seed(5))
    idx = ok.clone()
    where = torch.tensor([0, 137, 299], device=DEV)
    idx[where] = len(mem) if bad == "len" else bad
    ok[where] = 0
    dz, want = torch.empty(300, 2, device=DEV), torch.empty(300, 2, device=DEV)
    fused.update(mem, idx, dz_out=dz)
    clean.update(mem, ok, dz_out=want)
    assert fused.stats()["bad_index"] == 1 and clean.stats()["bad_index"] == 0
    assert bool(torch.isfinite(want).all()) and biteq(dz, want)
    for name in ("params", "grad", "adam_m", "adam_v", "rep_a"):
        assert biteq(getattr(fused, name), getattr(clean, name)), name
    fused.update(mem, ok)
    assert fused.stats()["bad_index"] == 1                                               # sticky


def same_trainer(a, b):
    for name in ("params", "grad", "adam_m", "adam_v", "rep_a", "state"):
        x, y = getattr(a, name), getattr(b, name)
        assert biteq(x.view(torch.int32), y.view(torch.int32)), name


def test_stale_scratch_does_not_leak_into_a_smaller_batch():
    mem, fused, _ = setup(seed=7)
    _, fresh, _ = setup(seed=7)
    g = torch.Generator(device=DEV).manual_seed(6)
    big, small = mem.sample_indices(256, g), mem.sample_indices(100, g)
    keep = {k: getattr(fused, k).clone() for k in ("params", "adam_m", "adam_v", "state", "rep_a")}
    fused.update(mem, big)
    for k, v in keep.items():                                                            # back to the start; the workspace stays dirty
        getattr(fused, k).copy_(v)
    fused.update(mem, small)
    poison_ws(fresh, 256)
    fresh.update(mem, small)
    same_trainer(fused, fresh)


def test_two_runs_are_bit_identical():
    runs = []
    for _ in range(2):
        mem, fused, _ = setup(seed=8, N=128)
        g = torch.Generator(device=DEV).manual_seed(7)
        for _ in range(5):
            fused.update(mem, mem.sample_indices(600, g))
        runs.append(fused)
    same_trainer(*runs)
    assert runs[0].stats()["steps"] == 5


# ---------------------------------------------------------------------------------------------------------------- the loop
def loop(n, steps, M=8, seed=11, batch=96, **hp):
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    teacher = rover_net(net(40))
    fused = D().FusedDAgger(net(41).state_dict(), **hp)
    mem = ReplayMemory(M, n, device=DEV)
    col = D().DAggerCollector(teacher, fused.actor, mem, seed=seed)
    data = Steps(n, steps, seed=seed)
    return teacher, fused, mem, col, [tuple(x.to(DEV) for x in data.at(t)) for t in range(steps + 1)], batch


def run(fused, col, data, betas, first=0, batch=96, begin=True):
    if begin:
        col.begin(data[first][0], data[first][1])
    acts = []
    for t, beta in enumerate(betas, start=first):
        acts.append(col.act(beta).clone())
        raw, dep, rew, term = data[t + 1]
        fused.update(col.memory, col.record(raw, dep, rew, term, batch))
    return acts


def test_resume_continues_bit_for_bit():
    betas = [1.0, 0.8, 0.6, 0.4, 0.2]
    teacher, fused, mem, col, data, batch = loop(48, 5)
    acts = run(fused, col, data, betas[:3])
    sd_t, sd_c, mem2 = fused.state_dict(), col.state_dict(), copy.deepcopy(mem)
    acts += run(fused, col, data, betas[3:], first=3, begin=False)
    again = D().FusedDAgger(net(99).state_dict())
    again.load_state_dict(sd_t)
    col2 = D().DAggerCollector(teacher, again.actor, mem2, seed=0)
    col2.load_state_dict(sd_c)
    rest = run(again, col2, data, betas[3:], first=3)             # begin() with the env's current rows refills the teacher's rows
    assert all(biteq(x, y) for x, y in zip(acts[3:], rest))
    same_trainer(fused, again)
    assert biteq(mem.obs, mem2.obs) and biteq(mem.actions, mem2.actions) and col.state_dict() == col2.state_dict()


def test_the_collector_sees_the_updated_student():
    teacher, fused, mem, col, data, batch = loop(40, 2, learning_rate=1e-2)
    a_s, first = torch.empty(40, 2, device=DEV), torch.empty(40, 2, device=DEV)
    col.begin(data[0][0], data[0][1])
    slot = mem.obs[mem.cursor].clone()
    col.act(0.0, student_out=first)
    fused.update(mem, col.record(*data[1], 64))
    mem.obs[mem.cursor].copy_(slot)                                # the same rows under the next act
    got = col.act(0.0, student_out=a_s).clone()
    assert biteq(a_s, fused.actor(slot)) and biteq(got, a_s) and not biteq(a_s, first)
    # ... which is the student of the checkpoint, evaluated by a network packed from scratch
    assert biteq(a_s, rover_net_from(fused.checkpoint())(slot))


def rover_net_from(ck):
    from isaac_rover_orbit_amd.policy import RoverNet
    return RoverNet.from_state_dict(ck["policy"], final_act="tanh")


def test_act_record_update_do_not_synchronise():
    teacher, fused, mem, col, data, batch = loop(64, 4)
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


def test_end_to_end_64_envs_30_steps():
    with time_limit(120):
        end_to_end()


def end_to_end():
    """The example's loop on the real env and camera: beta from 1 down to 0, one update per step; no claim about how well the student
    drives."""
    from isaac_rover_orbit_amd import terrain as T
    from isaac_rover_orbit_amd.cfg import RoverEnvCfg
    from isaac_rover_orbit_amd.envs import RoverEnv
    from isaac_rover_orbit_amd.policy import RoverNet
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    n, steps = 64, 30
    ter = T.make_procedural_terrain((512, 512), seed=21, n_rocks=40)
    ter.make_spawns(2 * n, border_offset=2.0)
    cfg = RoverEnvCfg()
    cfg.scene.num_envs, cfg.sim.device, cfg.terrain.kind, cfg.camera = n, "cuda:0", "custom", D().student_camera_cfg()
    env = RoverEnv(cfg, terrain=ter)
    teacher = rover_net(net(50))
    fused = D().FusedDAgger(net(51).state_dict())
    mem = ReplayMemory(16, n, device=DEV)
    col = D().DAggerCollector(teacher, fused.actor, mem, seed=3, env_id_offset=cfg.env_id_offset)
    obs, _ = env.reset()
    col.begin(obs, env.extras["depth"])
    losses = torch.empty(steps, device=DEV)
    for t in range(steps):
        obs, rew, term, trunc, _ = env.step(col.act(1.0 - t / (steps - 1)))
        fused.update(mem, col.record(obs, env.extras["depth"], rew, term, 128))
        losses[t] = fused.state.view(torch.float32)[2]             # rover_dagger_state.loss, copied on the device
    st = fused.stats()
    assert bool(torch.isfinite(losses).all()) and st["bad_index"] == 0 and st["steps"] == steps and mem.filled
    assert bool(torch.isfinite(fused.params).all())
    rows = mem.obs[mem.cursor].clone()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "student.pt")
        torch.save(fused.checkpoint(), path)
        loaded = RoverNet.from_checkpoint(path, role="policy")
        assert biteq(loaded(rows), fused.actor(rows))
        load_example().Net(2, True).load_state_dict(torch.load(path, map_location="cpu", weights_only=False)["policy"])
    env.close()
