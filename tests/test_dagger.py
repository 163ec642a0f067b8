"""The DAgger specification on the CPU (isaac_rover_orbit_amd/dagger.py): the student rows, the imitation loss with its closed-form
tanh backward, and the collector's mixing, sharding and checkpoint.  The kernels are held to these in test_gpu_dagger.py and, at the
draws' and the hyper-parameters' edges (the last section here), in test_gpu_dagger_collect_edges.py."""
import copy

import numpy as np
import pytest
import torch

from ppo_reference import load_example

NAN, INF = float("nan"), float("inf")


def D():
    from isaac_rover_orbit_amd import dagger
    return dagger


def student(seed=0, dtype=torch.float32):
    torch.manual_seed(seed)
    return load_example().Net(2, True).to(dtype)


def images(n, seed=0):
    """(n, 31, 31) render buffers with every special value planted."""
    g = torch.Generator().manual_seed(seed)
    d = torch.rand(n, 31, 31, generator=g) * 25.0
    flat = d.view(n, -1)
    for j, v in enumerate((NAN, INF, -INF, -1.0, 0.0, 10.0, 20.0, -0.0)):
        flat[:, (7 * j + 3) % 961] = v
        flat[j % n, 960 - j] = v
    return d


def env_rows(n, seed=0):
    g = torch.Generator().manual_seed(seed + 100)
    r = torch.randn(n, 965, generator=g)
    for j, v in enumerate((NAN, INF, -INF)):
        r[j % n, j % 4] = v
        r[(j + 1) % n, 4 + 11 * j] = v
    return r


# ---------------------------------------------------------------------------------------------------------------- rows
def test_student_camera_is_the_reference_camera_at_31_by_31():
    from isaac_rover_orbit_amd.cfg import CameraCfg
    cam, ref = D().student_camera_cfg(), CameraCfg()
    assert (cam.width, cam.height) == (31, 31)
    for k in ("focal_length", "horizontal_aperture", "vertical_aperture", "position", "orientation", "near_clip", "far_clip"):
        assert getattr(cam, k) == getattr(ref, k), k


def test_student_rows_special_pixels_and_clip():
    d = torch.zeros(1, 31, 31)
    vals = [NAN, INF, -INF, -1.0, -1e-30, 0.0, 10.0, 10.000001, 20.0, 9.999999, 3.0]
    d.view(-1)[:len(vals)] = torch.tensor(vals)
    rows = D().student_rows(d, torch.zeros(1, 965))
    clip = np.float32(0.1) * np.float32(10.0)
    want = [clip] * 5 + [0.0, clip, clip, clip, np.float32(0.1) * np.float32(9.999999), np.float32(0.1) * np.float32(3.0)]
    assert rows.dtype == torch.float32 and rows.shape == (1, 965)
    assert np.array_equal(rows[0, 4:4 + len(vals)].numpy(), np.array(want, np.float32))
    # hyper-parameters: another clip and scale
    rows = D().student_rows(d, torch.zeros(1, 965), depth_clip=5.0, depth_scale=2.0)
    assert rows[0, 4:4 + len(vals)].tolist() == [10.0] * 5 + [0.0] + [10.0] * 4 + [6.0]


def test_student_rows_layout_and_head_columns():
    n = 3
    d, e = images(n), env_rows(n)
    rows = D().student_rows(d, e)
    # columns 0..3: the env row's, sanitised by the collectors' rule; nothing else of the env row enters
    assert torch.equal(rows[:, :4], torch.nan_to_num(e[:, :4], nan=0.0, posinf=float(np.finfo(np.float32).max), neginf=0.0))
    assert torch.isfinite(rows).all()
    e2 = e.clone(); e2[:, 4:] = 7.0
    assert torch.equal(D().student_rows(d, e2), rows)
    # column 4 + p is pixel p of the row-major (height, width) buffer: pixel (h, w) sits at 4 + 31 h + w
    probe = torch.full((1, 31, 31), 1.0)
    probe[0, 2, 5] = 4.0
    r = D().student_rows(probe, torch.zeros(1, 965))
    assert r[0, 4 + 31 * 2 + 5] == np.float32(0.1) * np.float32(4.0) and (r[0, 4:] != np.float32(0.1)).sum() == 1
    # the env's extras["depth"] is the (n, width, height) permuted view of that buffer: same rows, no copy
    view = d.permute(0, 2, 1)
    assert not view.is_contiguous() and D().image_buffer(view).data_ptr() == d.data_ptr()
    assert torch.equal(D().student_rows(view, e), rows)
    with pytest.raises(ValueError):
        D().student_rows(torch.zeros(n, 90, 160), e)


def test_last_pixel_is_never_read():
    net = student()
    d, e = images(4), env_rows(4)
    rows = D().student_rows(d, e)
    d2 = d.clone(); d2[:, 30, 30] = 0.123
    rows2 = D().student_rows(d2, e)
    assert not torch.equal(rows2[:, 964], rows[:, 964]) and torch.equal(rows2[:, :964], rows[:, :964])
    with torch.no_grad():
        assert torch.equal(net(rows), net(rows2))
        d3 = d.clone(); d3[:, 30, 29] = 0.123          # the pixel before it is read
        assert not torch.equal(net(D().student_rows(d3, e)), net(rows))


# ---------------------------------------------------------------------------------------------------------------- loss
def test_closed_form_dz_is_autograds_gradient():
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(37, 2, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    labels = torch.rand(37, 2, generator=g, dtype=torch.float64) * 2 - 1
    loss = D().imitation_loss(torch.tanh(z), labels)
    assert float(loss.detach()) == pytest.approx(float(((torch.tanh(z.detach()) - labels) ** 2).sum() / (2 * 37)), rel=1e-15)
    (auto,) = torch.autograd.grad(loss, z)
    closed = D().imitation_dz(torch.tanh(z).detach(), labels)
    assert torch.allclose(closed, auto, rtol=1e-12, atol=1e-15)


def filled_memory(n=8, steps=4, seed=5):
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    mem = ReplayMemory(steps, n, device="cpu")
    g = torch.Generator().manual_seed(seed)
    s = D().student_rows(images(n, seed), env_rows(n, seed))
    for t in range(steps):
        s2 = D().student_rows(images(n, seed + t + 1), env_rows(n, seed + t + 1))
        mem.add(s, torch.rand(n, 2, generator=g) * 2 - 1, torch.zeros(n, 1), s2, torch.zeros(n, 1, dtype=torch.bool))
        s = s2
    return mem


def test_torch_dagger_dz_matches_autograd_and_the_loss_falls():
    mem = filled_memory()
    idx = torch.arange(32)
    spec = D().TorchDAgger(student(1, torch.float64))
    s, a, *_ = mem.gather(idx)
    # the closed form against autograd through the network's own tanh
    pre = {}
    h = spec.student.mlp[6].register_forward_hook(lambda m, i, o: pre.setdefault("z", o))
    out = spec.student(s.double())
    h.remove()
    (auto,) = torch.autograd.grad(D().imitation_loss(out, a.double()), pre["z"])
    assert torch.allclose(D().imitation_dz(out.detach(), a.double()), auto, rtol=1e-10, atol=1e-15)
    losses = [spec.update(mem, idx)["loss"] for _ in range(51)]
    assert all(np.isfinite(losses)) and losses[50] < losses[0]
    assert "policy" in spec.checkpoint() and "mlp.6.weight" in spec.checkpoint()["policy"]


def test_grad_norm_clip_scales_the_gradient_and_reports_the_unclipped_norm():
    mem = filled_memory()
    idx = torch.arange(32)
    a, b = D().TorchDAgger(student(2, torch.float64)), D().TorchDAgger(student(2, torch.float64), grad_norm_clip=1e-3)
    sa, sb = a.update(mem, idx), b.update(mem, idx)
    assert sa["grad_norm"] == pytest.approx(sb["grad_norm"]) and sa["grad_norm"] > 1e-3
    ga, gb = a.student.mlp[6].weight.grad, b.student.mlp[6].weight.grad
    assert torch.allclose(gb, ga * (1e-3 / (sa["grad_norm"] + 1e-6)), rtol=1e-12, atol=0)
    with pytest.raises(TypeError):
        D().TorchDAgger(student(), no_such=1)


# ---------------------------------------------------------------------------------------------------------------- collector
class Steps:
    """A fixed sequence of (raw rows, depth, reward, terminated) for n envs; ``part(lo, hi)`` cuts the envs of a shard."""

    def __init__(self, n, steps, seed=9):
        self.n = n
        self.data = [(env_rows(n, seed + t), images(n, seed + t), torch.randn(n, generator=torch.Generator().manual_seed(t)),
                      torch.arange(n) % (t + 2) == 0) for t in range(steps + 1)]

    def at(self, t, lo=0, hi=None):
        return tuple(x[lo:hi].contiguous() for x in self.data[t])


def collector(n, teacher, stud, offset=0, M=6, seed=(3 << 32) | 11):
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    return D().TorchDAggerCollector(teacher, stud, ReplayMemory(M, n, device="cpu"), seed=seed, env_id_offset=offset)


def drive(col, steps, betas, lo=0, hi=None, first=0, begin=True, batch=16):
    out = []
    if begin:
        raw, dep, _, _ = steps.at(first, lo, hi)
        col.begin(raw, dep)
    for t, beta in enumerate(betas, start=first):
        a = col.act(beta).clone()
        raw, dep, rew, term = steps.at(t + 1, lo, hi)
        idx = col.record(raw, dep, rew, term, batch)
        out.append((a, col.last["label"].clone(), col.last["student"].clone(), col.last["source"].clone(), idx))
    return out


def test_beta_edges_are_exact_and_labels_are_stored():
    n = 12
    teacher, stud = student(20), student(21)
    steps = Steps(n, 3)
    for beta, who in ((1.0, 1), (0.0, 2)):
        col = collector(n, teacher, stud)
        for t, rec in enumerate(drive(col, steps, [beta] * 3)):
            assert torch.equal(rec[0], rec[who]) and bool(rec[3].all()) == (beta == 1.0) and bool(rec[3].any()) == (beta == 1.0)
            raw, dep, _, _ = steps.at(t)
            with torch.no_grad():
                assert torch.equal(rec[1], teacher(D().sanitise(raw)))                     # the teacher reads the sanitised env row
                assert torch.equal(rec[2], stud(D().student_rows(dep, raw)))               # the student its own rows
            assert torch.equal(col.memory.actions[t], rec[1])                              # the label, whoever drove
        assert col.counter == 6 and len(col.memory) == 3 * n
    # in between: both sources occur, each env takes exactly the one its draw names
    col = collector(n, teacher, stud)
    u = col.draws()
    (rec,) = drive(col, Steps(n, 1), [0.5])
    src = torch.from_numpy(u < 0.5)
    assert 0 < int(src.sum()) < n and torch.equal(rec[3], src)
    assert torch.equal(rec[0], torch.where(src.unsqueeze(1), rec[1], rec[2]))
    with pytest.raises(ValueError):
        col.act(1.5)


def test_two_shards_reproduce_the_unsplit_run():
    n, cut = 10, 4
    # row-wise callables: a BLAS product may round a row differently in a batch of another size, which is not what is pinned here
    teacher = lambda rows: torch.tanh(rows[:, 1:3] + rows[:, 7:9])          # noqa: E731
    stud = lambda rows: torch.tanh(rows[:, 0:2] - rows[:, 400:402])         # noqa: E731
    steps, betas = Steps(n, 4), [0.7, 0.5, 0.3, 0.1]
    whole = drive(collector(n, teacher, stud, offset=100), steps, betas)
    a = drive(collector(cut, teacher, stud, offset=100), steps, betas, 0, cut)
    b = drive(collector(n - cut, teacher, stud, offset=100 + cut), steps, betas, cut, n)
    mixed = 0
    for w, x, y in zip(whole, a, b):
        for k in range(4):
            assert torch.equal(w[k], torch.cat([x[k], y[k]]))
        mixed += int(w[3].sum())
    assert 0 < mixed < 4 * n


def test_checkpoint_after_step_2_reproduces_steps_3_and_4():
    n = 9
    teacher, stud = student(24), student(25)
    steps, betas = Steps(n, 4), [0.6, 0.4, 0.5, 0.5]
    col = collector(n, teacher, stud)
    full = drive(col, steps, betas[:2])
    sd, mem = col.state_dict(), copy.deepcopy(col.memory)
    assert sd == {"seed": (3 << 32) | 11, "counter": 4, "env_id_offset": 0}
    full += drive(col, steps, betas[2:], first=2, begin=False)
    again = D().TorchDAggerCollector(teacher, stud, mem, seed=1)
    again.load_state_dict(sd)
    rest = drive(again, steps, betas[2:], first=2)           # begin() with the env's current rows rewrites the cursor slot
    for w, x in zip(full[2:], rest):
        for k in range(5):
            assert torch.equal(w[k], x[k])
    assert torch.equal(again.memory.obs, col.memory.obs) and torch.equal(again.memory.actions, col.memory.actions)
    # the indices are the TD3 collector's stream under the same seed and counter
    from isaac_rover_orbit_amd.td3_collect import sample_indices
    assert np.array_equal(full[3][4].numpy(), sample_indices((3 << 32) | 11, 7, 16, 4 * n))


# ---------------------------------------------------------------------------------------------------------------- edges
def test_mix_uniforms_equal_the_by_hand_philox_at_the_top_of_the_ranges():
    """The specification the kernel's draw is held to, against Philox in Python integers: ids up to 2**31 - 2, every key bit set,
    counters around 2**32 and at 2**64 - 1.  Exact: u = (k + 0.5) * 2**-23 is a float32."""
    from dagger_helpers import mix_uniforms_by_hand
    from td3_helpers import TOP_COUNTERS, TOP_OFFSET, TOP_SEED
    ids = TOP_OFFSET + np.arange(33)
    assert ids[-1] == 2 ** 31 - 2
    seen = []
    for counter in TOP_COUNTERS:
        u = D().mix_uniforms(TOP_SEED, ids, counter)
        assert u.dtype == np.float32 and u.tolist() == mix_uniforms_by_hand(TOP_SEED, ids, counter)
        assert len(set(u.tolist())) == 33 and 0 < int((u < 0.5).sum()) < 33 and u.min() >= 2.0 ** -24 and u.max() < 1.0
        seen.append((u < 0.5).tolist())
    assert seen[0] != seen[1] != seen[2] != seen[0]
    # another id, seed or counter word is another draw
    base = D().mix_uniforms(TOP_SEED, ids, TOP_COUNTERS[0])
    assert not np.array_equal(base, D().mix_uniforms(TOP_SEED, ids - 1, TOP_COUNTERS[0]))
    assert not np.array_equal(base, D().mix_uniforms(TOP_SEED ^ (1 << 63), ids, TOP_COUNTERS[0]))


def test_beta_on_a_draw_takes_the_student():
    """The mix is u < beta: with beta = u_k env k takes the student, with the next float32 the teacher, nobody else moves."""
    n, k = 33, 16
    teacher = lambda rows: torch.tanh(rows[:, 1:3] + rows[:, 7:9])          # noqa: E731
    stud = lambda rows: torch.tanh(rows[:, 0:2] - rows[:, 400:402])         # noqa: E731
    steps = Steps(n, 1)
    u = collector(n, teacher, stud, offset=7).draws()
    assert u.dtype == np.float32 and len(set(u.tolist())) == n
    on, after = float(u[k]), float(np.nextafter(u[k], np.float32(1.0)))
    got = {}
    for beta in (on, after):
        col = collector(n, teacher, stud, offset=7)
        (rec,) = drive(col, steps, [beta])
        src = rec[3].numpy()
        assert np.array_equal(np.delete(src, k), np.delete(u < on, k)) and 0 < int(src.sum()) < n
        assert torch.equal(rec[0], torch.where(rec[3].unsqueeze(1), rec[1], rec[2])) and not torch.equal(rec[1][k], rec[2][k])
        got[beta] = bool(src[k])
    assert got == {on: False, after: True}
    # the smallest possible draw is 2**-24: that beta takes no teacher at all
    col = collector(n, teacher, stud, offset=7)
    (rec,) = drive(col, steps, [2.0 ** -24])
    assert not bool(rec[3].any())


@pytest.mark.parametrize("scale", [0.0, -0.1, INF, 1e-45])
def test_student_rows_at_degenerate_depth_scales(scale):
    d, e = images(3), env_rows(3)
    rows = D().student_rows(d, e, depth_scale=scale)
    s = np.float32(scale)
    flat = d.view(3, -1).numpy()
    with np.errstate(invalid="ignore"):
        pix = np.where(np.isnan(flat) | np.isinf(flat) | (flat < 0), np.float32(10.0), flat)
        want = s * np.minimum(pix, np.float32(10.0))
    got = rows[:, 4:].numpy()
    assert got.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~np.isnan(got)].view(np.uint32), want[~np.isnan(want)].astype(np.float32).view(np.uint32))
    zero = flat == 0
    assert zero.any()
    if scale == INF:
        assert np.isnan(got[zero]).all() and np.isinf(got[~zero]).all()          # inf * 0: the zero pixels are NaN, as in torch
    elif scale == 0.0:
        assert not got.any()
    elif scale == 1e-45:
        assert s > 0 and float(got.max()) == float(s * np.float32(10.0)) > 0      # a denormal scale is a number, not flushed
    else:
        assert float(got.max()) == 0.0 and float(got.min()) == float(s * np.float32(10.0))
    assert torch.equal(rows[:, :4], D().sanitise(e[:, :4]))


@pytest.mark.parametrize("clip", [1e-45, float(np.finfo(np.float32).max)])
def test_student_rows_at_the_ends_of_depth_clip(clip):
    d, e = images(3), env_rows(3)
    rows = D().student_rows(d, e, depth_clip=clip)
    c = np.float32(clip)
    flat = d.view(3, -1).numpy()
    got = rows[:, 4:].numpy()
    assert np.isfinite(got).all() and float(got.max()) == float(np.float32(0.1) * c)
    bad = np.isnan(flat) | np.isinf(flat) | (flat < 0)
    assert (got[bad] == np.float32(0.1) * c).all() and (got[flat == 0] == 0).all()
    if clip < 1.0:                                                              # every positive pixel is above the smallest denormal
        assert (got[flat > 0] == np.float32(0.1) * c).all()
    else:                                                                       # nothing is clipped but what is not a depth
        ok = ~bad
        assert np.array_equal(got[ok], np.float32(0.1) * flat[ok])
