"""The 160 x 90 DAgger student's specification on the CPU (isaac_rover_orbit_amd/dagger_conv.py): the convolutional stem against
torch's conv2d, its padding, its closed-form backward, the never-read last feature, the joint clip, and the collector's sharding and
checkpoint.  The kernels are held to these in test_gpu_dagger_conv.py."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_dagger import env_rows, student

NAN, INF = float("nan"), float("inf")
SPECIALS = (NAN, INF, -INF, -1.0, 0.0, 10.0, 20.0, -0.0)


def DC():
    from isaac_rover_orbit_amd import dagger_conv
    return dagger_conv


def stem(seed=0, dtype=torch.float64, both_signs=True):
    m = DC().ConvStem.seeded(seed).to(dtype)
    if both_signs:                       # weights and biases of both signs and of a size that puts pre-activations on both branches
        with torch.no_grad():
            g = torch.Generator().manual_seed(seed + 50)
            m.conv1.weight.copy_(torch.randn(m.conv1.weight.shape, generator=g, dtype=dtype) * 0.2)
            m.conv1.bias.copy_(torch.randn(8, generator=g, dtype=dtype) * 0.3)
            m.conv2.weight.copy_(torch.randn(m.conv2.weight.shape, generator=g, dtype=dtype))
    return m


def images(n, seed=0, kind="random"):
    """(n, 90, 160) render buffers in metres.  ``random``: every special value on window corners (rows 3 i, columns 5 j and the cells
    before them), in the first and last image rows and columns."""
    g = torch.Generator().manual_seed(seed)
    if kind == "clip":
        return torch.full((n, 90, 160), 25.0)
    if kind == "ramp":
        return (torch.arange(90 * 160, dtype=torch.float32).reshape(1, 90, 160) * (12.0 / 14400) + torch.arange(n).view(n, 1, 1)).contiguous()
    d = torch.rand(n, 90, 160, generator=g) * 25.0
    for k, v in enumerate(SPECIALS):
        e = k % n
        d[e, 0, 7 * k] = v; d[e, 89, 159 - 7 * k] = v; d[e, 11 * k, 0] = v; d[e, 89 - 11 * k, 159] = v
        d[e, 3 * (k + 1), 5 * (k + 2)] = v; d[e, 3 * (k + 1) - 1, 5 * (k + 2) - 1] = v           # a window's first cell; the cell before it
        d[(e + 1) % n, 3 * k + 5, 5 * k + 9] = v; d[(e + 1) % n, 3 * k + 6, 5 * k + 10] = v       # a window's last cell; the one behind it
    return d


# ---------------------------------------------------------------------------------------------------------------- the stem
def test_output_is_31_by_31_and_other_sizes_are_refused():
    m = stem(0, torch.float32)
    x = torch.rand(2, 90, 160)
    assert tuple(m(x).shape) == (2, 961) and DC().STEM_FLOATS == 497 == m.packed().numel()
    assert tuple(m.conv1(x.unsqueeze(1)).shape) == (2, 8, 31, 31)
    cam = DC().student_camera_cfg()
    assert (cam.width, cam.height) == (160, 90)
    for bad in (torch.rand(2, 31, 31), torch.rand(2, 160, 90), torch.rand(2, 91, 160), torch.rand(2, 90, 161)):
        with pytest.raises(ValueError):
            m(bad)
        with pytest.raises(ValueError):
            DC().conv_student_rows(m, bad, torch.zeros(2, 965))
    # the env's extras["depth"] is the (n, 160, 90) permuted view of the (n, 90, 160) buffer: taken back without a copy
    buf = torch.rand(2, 90, 160)
    assert DC().image_buffer(buf.permute(0, 2, 1)).data_ptr() == buf.data_ptr()
    assert torch.equal(DC().conv_student_rows(m, buf.permute(0, 2, 1), torch.zeros(2, 965)), DC().conv_student_rows(m, buf, torch.zeros(2, 965)))


def test_stem_is_conv2d_with_the_stated_stride_and_padding():
    m = stem(1)
    x = torch.rand(3, 90, 160, dtype=torch.float64)
    h = F.leaky_relu(F.conv2d(x.unsqueeze(1), m.conv1.weight, m.conv1.bias, stride=(3, 5), padding=(3, 0)), 0.01)
    y = F.conv2d(h, m.conv2.weight, m.conv2.bias)
    assert bool((h > 0).any()) and bool((h < 0).any())
    assert torch.equal(m(x), y.reshape(3, 961))
    # feature 31 i + j is y(i, j); the packed layout is W1[8][6][10], b1[8], w2[8], b2 and survives a round trip
    assert torch.equal(m(x)[:, 31 * 4 + 7], y[:, 0, 4, 7])
    p = m.packed()
    m.requires_grad_(False)
    assert float(p[2 * 60 + 3 * 10 + 4]) == float(m.conv1.weight[2, 0, 3, 4]) and float(p[480 + 5]) == float(m.conv1.bias[5])
    assert float(p[488 + 6]) == float(m.conv2.weight[0, 6, 0, 0]) and float(p[496]) == float(m.conv2.bias[0])
    assert torch.equal(DC().ConvStem.from_packed(p, torch.float64)(x), m(x))


def test_special_pixels_and_both_clip_edges():
    d = torch.zeros(1, 90, 160)
    vals = [NAN, INF, -INF, -1.0, -1e-30, 0.0, 10.0, 10.000001, 20.0, 9.999999, 3.0]
    d.view(-1)[:len(vals)] = torch.tensor(vals)
    x = DC().preprocess(d)
    clip = np.float32(0.1) * np.float32(10.0)
    want = [clip] * 5 + [0.0, clip, clip, clip, np.float32(0.1) * np.float32(9.999999), np.float32(0.1) * np.float32(3.0)]
    assert x.dtype == torch.float32 and np.array_equal(x.view(-1)[:len(vals)].numpy(), np.array(want, np.float32))
    assert DC().preprocess(d, 5.0, 2.0).view(-1)[:len(vals)].tolist() == [10.0] * 5 + [0.0] + [10.0] * 4 + [6.0]
    # the rows: columns 0..3 are the sanitised env row's, nothing else of the env row enters, everything is finite
    m, e = stem(2, torch.float32), env_rows(3)
    rows = DC().conv_student_rows(m, images(3), e)
    assert rows.shape == (3, 965) and bool(torch.isfinite(rows).all())
    assert torch.equal(rows[:, :4], torch.nan_to_num(e[:, :4], nan=0.0, posinf=float(np.finfo(np.float32).max), neginf=0.0))
    e2 = e.clone(); e2[:, 4:] = 7.0
    assert torch.equal(DC().conv_student_rows(m, images(3), e2), rows)


def test_padded_taps_contribute_nothing():
    m = stem(3)
    x = torch.rand(2, 90, 160, dtype=torch.float64) + 0.5
    y = m(x).detach().view(2, 31, 31)
    w1, b1 = m.conv1.weight.detach()[:, 0], m.conv1.bias.detach()
    w2, b2 = m.conv2.weight.detach().view(8), m.conv2.bias.detach()

    def by_hand(i, j, rows_u):
        pre = b1.clone()
        for u in rows_u:
            pre = pre + (w1[:, u, :] * x[0, 3 * i - 3 + u, 5 * j:5 * j + 10]).sum(1)
        return float(b2 + (w2 * torch.where(pre > 0, pre, 0.01 * pre)).sum())

    # outputs i = 0 and i = 30 are a sum over their three real rows: kernel rows 3..5 on image rows 0..2, kernel rows 0..2 on 87..89
    for j in (0, 13, 30):
        assert float(y[0, 0, j]) == pytest.approx(by_hand(0, j, (3, 4, 5)), rel=1e-12)
        assert float(y[0, 30, j]) == pytest.approx(by_hand(30, j, (0, 1, 2)), rel=1e-12)
        assert float(y[0, 7, j]) == pytest.approx(by_hand(7, j, range(6)), rel=1e-12)
    # the same image inside a taller canvas, convolved without padding: whatever the canvas holds where the padding would be,
    # outputs 1..29 do not move (they read no padded position) and with zeros there the whole output is the stem's
    def canvas(fill):
        c = torch.cat([torch.full((2, 3, 160), fill, dtype=torch.float64), x, torch.full((2, 3, 160), fill, dtype=torch.float64)], 1)
        h = F.leaky_relu(F.conv2d(c.unsqueeze(1), m.conv1.weight, m.conv1.bias, stride=(3, 5)), 0.01)
        return F.conv2d(h, m.conv2.weight, m.conv2.bias).detach().view(2, 31, 31)
    assert torch.equal(canvas(0.0), y)
    junk = canvas(123.0)
    assert torch.equal(junk[:, 1:30], y[:, 1:30]) and not torch.equal(junk[:, 0], y[:, 0]) and not torch.equal(junk[:, 30], y[:, 30])
    # ... and in the backward: the gradient of W1's rows 0..2 holds nothing of output row 0
    g = torch.zeros(2, 961, dtype=torch.float64); g[:, :31] = 1.0
    grads = DC().stem_backward(m, x, g)
    assert bool((grads["conv1.weight"][:, 0, :3] == 0).all()) and bool((grads["conv1.weight"][:, 0, 3:] != 0).any())


def test_closed_form_backward_is_autograds():
    m = stem(4)
    x = torch.rand(4, 90, 160, dtype=torch.float64)
    x[3] = 0.0                                       # an image of zeros: every pre-activation is its bias ...
    with torch.no_grad():
        m.conv1.bias[0] = 0.0                        # ... and channel 0's is exactly 0: the derivative there is the slope
    g = torch.randn(4, 961, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    pre = F.conv2d(x.unsqueeze(1), m.conv1.weight, m.conv1.bias, stride=(3, 5), padding=(3, 0))
    assert bool((pre[3, 0] == 0).all()) and bool((pre[:3] > 0).any()) and bool((pre[:3] < 0).any())
    (m(x) * g).sum().backward()
    closed = DC().stem_backward(m, x, g)
    for k, p in m.named_parameters():
        assert torch.allclose(closed[k], p.grad, rtol=1e-11, atol=1e-13), k
    # at pre = 0 the slope: channel 0's share of db1 from the zero image is 0.01 * w2[0] * sum g
    only = DC().stem_backward(m, x[3:], g[3:])
    assert float(only["conv1.bias"][0]) == pytest.approx(0.01 * float(m.conv2.weight.detach()[0, 0, 0, 0]) * float(g[3].sum()), rel=1e-12)


def test_feature_30_30_is_never_read():
    head, m = student(1, torch.float64), stem(5)
    d, e = images(3), env_rows(3).double()
    rows = DC().conv_student_rows(m, d, e).detach().requires_grad_(True)
    head(rows).sum().backward()
    assert bool((rows.grad[:, 964] == 0).all()) and bool((rows.grad[:, 963] != 0).any())
    with torch.no_grad():
        moved = rows.detach().clone(); moved[:, 964] += 5.0
        assert torch.equal(head(moved), head(rows))
        moved = rows.detach().clone(); moved[:, 963] += 5.0
        assert not torch.equal(head(moved), head(rows))


# ---------------------------------------------------------------------------------------------------------------- the trainer
def pairs(n=16, seed=7):
    g = torch.Generator().manual_seed(seed)
    x = DC().preprocess(images(n, seed)).double()
    env4 = torch.randn(n, 4, generator=g, dtype=torch.float64)
    labels = torch.rand(n, 2, generator=g, dtype=torch.float64) * 2 - 1
    return env4, x, labels


def test_joint_clip_is_clip_grad_norm_over_both_lists():
    env4, x, labels = pairs()
    a = DC().TorchConvDAgger(student(2, torch.float64), stem(6, both_signs=False))
    b = DC().TorchConvDAgger(student(2, torch.float64), stem(6, both_signs=False), grad_norm_clip=1e-3)
    sa, sb = a.step(env4, x, labels), b.step(env4, x, labels)
    every = [p.grad for p in a._head_params] + [p.grad for p in a._stem_params]
    joint = float(torch.sqrt(sum((g.double() ** 2).sum() for g in every)))
    head_only = float(torch.sqrt(sum((p.grad ** 2).sum() for p in a._head_params)))
    assert sa["grad_norm"] == pytest.approx(joint, rel=1e-12) and sa["grad_norm"] == pytest.approx(sb["grad_norm"], rel=1e-12)
    assert joint > head_only > 1e-3
    coef = 1e-3 / (joint + 1e-6)
    for pa, pb in zip(a._params, b._params):
        assert torch.allclose(pb.grad, pa.grad * coef, rtol=1e-12, atol=0)
    # what torch's own clip over both lists leaves
    c = DC().TorchConvDAgger(student(2, torch.float64), stem(6, both_signs=False))
    rows = c.rows(env4, x)
    DC().imitation_loss(c.student(rows), labels).backward()
    total = torch.nn.utils.clip_grad_norm_(c._head_params + c._stem_params, 1e-3)
    assert float(total) == pytest.approx(joint, rel=1e-12)
    for pc, pb in zip(c._params, b._params):
        assert torch.allclose(pc.grad, pb.grad, rtol=1e-12, atol=0)
    with pytest.raises(TypeError):
        DC().TorchConvDAgger(student(), stem(), no_such=1)


def test_fifty_steps_on_sixteen_pairs_lower_the_loss():
    env4, x, labels = pairs(16)
    spec = DC().TorchConvDAgger(student(3, torch.float64), stem(7, both_signs=False))
    before = spec.stem.packed().clone()
    losses = [spec.step(env4, x, labels)["loss"] for _ in range(51)]
    assert all(np.isfinite(losses)) and losses[50] < losses[0]
    assert not torch.equal(spec.stem.packed(), before)                      # the stem learns too
    ck = spec.checkpoint()
    assert "mlp.6.weight" in ck["policy"] and set(ck[DC().STEM_KEY]) == {"conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"}


# ---------------------------------------------------------------------------------------------------------------- collector
class Steps:
    """A fixed sequence of (raw rows, depth, reward, terminated) for n envs."""

    def __init__(self, n, steps, seed=9):
        self.n = n
        self.data = [(env_rows(n, seed + t), images(n, seed + t), torch.randn(n, generator=torch.Generator().manual_seed(t)),
                      torch.arange(n) % (t + 2) == 0) for t in range(steps + 1)]

    def at(self, t, lo=0, hi=None):
        return tuple(x[lo:hi].contiguous() for x in self.data[t])


# row-wise callables: a BLAS or conv product may round a row differently in a batch of another size, which is not what is pinned here
def teacher_fn(rows):
    return torch.tanh(rows[:, 1:3] + rows[:, 7:9])


def student_fn(rows):
    return torch.tanh(rows[:, 0:2] - rows[:, 400:402])


def stem_fn(x):
    return x.reshape(x.shape[0], 90, 32, 5).sum(3)[:, 1:, :31].reshape(x.shape[0], -1)[:, :961] * 0.2


def collector(n, offset=0, M=6, seed=(3 << 32) | 11):
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    return DC().TorchConvDAggerCollector(teacher_fn, student_fn, stem_fn, ReplayMemory(M, n, device="cpu"), DC().ImageRing(M, n, "cpu"),
                                         seed=seed, env_id_offset=offset)


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


def test_collector_fills_both_rings_and_two_shards_reproduce_the_unsplit_run():
    n, cut = 10, 4
    steps, betas = Steps(n, 4), [0.7, 0.5, 0.3, 0.1]
    col = collector(n, offset=100)
    whole = drive(col, steps, betas)
    # the image ring holds x of the step whose rows the observation ring holds, slot for slot
    for t in range(5):
        raw, dep, _, _ = steps.at(t)
        assert torch.equal(col.images.x[t].view(n, 90, 160), DC().preprocess(dep))
        assert torch.equal(col.memory.obs[t], torch.cat([DC().sanitise(raw[:, :4]), stem_fn(DC().preprocess(dep))], 1))
    idx = torch.tensor([0, 13, 39])
    assert torch.equal(col.images.gather(col.memory, idx)[1], DC().preprocess(steps.at(1)[1])[3])
    a = drive(collector(cut, offset=100), steps, betas, 0, cut)
    b = drive(collector(n - cut, offset=100 + cut), steps, betas, cut, n)
    mixed = 0
    for w, x, y in zip(whole, a, b):
        for k in range(4):
            assert torch.equal(w[k], torch.cat([x[k], y[k]]))
        mixed += int(w[3].sum())
    assert 0 < mixed < 4 * n
    with pytest.raises(ValueError):
        from isaac_rover_orbit_amd.td3 import ReplayMemory
        DC().TorchConvDAggerCollector(teacher_fn, student_fn, stem_fn, ReplayMemory(6, n, device="cpu"), DC().ImageRing(5, n, "cpu"))


def test_checkpoint_after_step_2_reproduces_steps_3_and_4():
    n = 9
    steps, betas = Steps(n, 4), [0.6, 0.4, 0.5, 0.5]
    col = collector(n)
    full = drive(col, steps, betas[:2])
    sd, mem, ring = col.state_dict(), copy.deepcopy(col.memory), copy.deepcopy(col.images)
    counters = DC().ring_counters(col.memory)
    assert sd == {"seed": (3 << 32) | 11, "counter": 4, "env_id_offset": 0} and counters == {"memory_index": 2, "filled": False, "cursor": 2}
    full += drive(col, steps, betas[2:], first=2, begin=False)
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    fresh = ReplayMemory(6, n, device="cpu")
    for k in ("obs", "actions", "rewards", "terminated", "ring_pos"):
        getattr(fresh, k).copy_(getattr(mem, k))
    DC().load_ring_counters(fresh, counters)
    again = DC().TorchConvDAggerCollector(teacher_fn, student_fn, stem_fn, fresh, ring, seed=1)
    again.load_state_dict(sd)
    rest = drive(again, steps, betas[2:], first=2)           # begin() with the env's current rows rewrites the cursor slot
    for w, x in zip(full[2:], rest):
        for k in range(5):
            assert torch.equal(w[k], x[k])
    assert torch.equal(again.memory.obs, col.memory.obs) and torch.equal(again.memory.actions, col.memory.actions)
    assert torch.equal(again.images.x, col.images.x)
    # resume(): the teacher's rows alone, both rings untouched
    third = DC().TorchConvDAggerCollector(teacher_fn, student_fn, stem_fn, copy.deepcopy(mem), copy.deepcopy(ring), seed=1)
    DC().load_ring_counters(third.memory, counters)
    third.load_state_dict(sd)
    kept = third.memory.obs.clone()
    third.resume(steps.at(2)[0])
    assert torch.equal(third.memory.obs, kept) and torch.equal(third.teacher_rows, DC().sanitise(steps.at(2)[0]))
    for w, x in zip(full[2:], drive(third, steps, betas[2:], first=2, begin=False)):
        for k in range(5):
            assert torch.equal(w[k], x[k])


# ---------------------------------------------------------------------------------------------------------------- the build
def test_stem_kernels_use_no_scratch_and_fit_two_workgroups_per_cu():
    """The three stem kernels keep everything in registers (no private segment), run as 512-thread workgroups and leave room for two
    workgroups in a CU's 160 KiB of LDS; the C ABI names its constants as the Python module does."""
    import re
    import subprocess
    import tempfile
    import os
    from helpers import gfx950_code_objects
    from isaac_rover_orbit_amd import _lib, build
    build.build_extension()
    lib = _lib.load()
    assert lib.rover_dagger_conv_stem_floats() == DC().STEM_FLOATS and lib.rover_dagger_conv_chunk_rows() == 8
    assert lib.rover_dagger_conv_workspace_bytes(0) == 0 and lib.rover_dagger_conv_workspace_bytes(1) > 2 * 965 * 4
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("ROCm llvm tools not installed")
    seen = {}
    for blob in gfx950_code_objects(_lib.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True).stdout
        for entry in re.split(r"\n\s*- \.", notes):
            m = re.search(r"\.name:\s*\S*(rover_dagger_conv_rows_kernel|dagger_conv_forward_kernel|dagger_conv_backward_kernel)\S*", entry)
            if not m or ".private_segment_fixed_size" not in entry:
                continue
            seen[m.group(1)] = int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", entry).group(1))
            assert re.search(r"\.private_segment_fixed_size:\s*0\b", entry), f"{m.group(1)} uses scratch memory"
            assert re.search(r"\.max_flat_workgroup_size:\s*512\b", entry), m.group(1)
            assert int(re.search(r"\.vgpr_count:\s*(\d+)", entry).group(1)) <= 128, f"{m.group(1)}: four waves per SIMD need <= 128 VGPRs"
    assert set(seen) == {"rover_dagger_conv_rows_kernel", "dagger_conv_forward_kernel", "dagger_conv_backward_kernel"}, seen
    assert seen["dagger_conv_forward_kernel"] == seen["rover_dagger_conv_rows_kernel"] == 96 * 160 * 4
    assert all(2 * v <= 160 * 1024 for v in seen.values()), seen
