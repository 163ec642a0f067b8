"""The fused DAgger collector (include/rover_dagger.h, csrc/dagger_collect_kernels.hip) at the branches tests/test_gpu_dagger.py does
not reach.  At most 97 rows per case (112 for the replicas); every output sits between sentinel guards that are checked after every
launch.  Every comparison is on the bits (NaN-aware where a NaN is the right answer); there is no tolerance in this file.

  * rows: n in {2, 3, 5} (2, 3 and 1 floats behind the last 16-byte piece); each of the four pointers 4, 8 and 12 bytes off a 16-byte
    boundary alone, all four together, aligned, and without the teacher's rows; the special values on the env columns, on the pixels
    of the pieces that straddle a row's head (0 .. 3, 957 .. 960) and on the buffer's last two floats, every value at every place
    on the vector path; against dagger.student_rows and dagger.sanitise
  * rows: depth_scale 0, negative, infinite (0 * inf is NaN, as in torch) and denormal; depth_clip denormal and FLT_MAX
  * record: indices at mem_rows 2**31, 2**32 - 1, 2**32 with batches 3, 5, 1023, 1025 over one row (the batch sizes the grid) and 3
    over 97 rows, seed 2**64 - 1, counters 2**32 - 1 and 2**64 - 1: equal to td3_collect.sample_indices, to the indices of
    rover_td3_collect_record, and in range; terminated bytes 0, 1, 2, 255; ring_pos; the slot
  * act: beta on a draw takes the student and the next float32 the teacher (the comparison is strict); beta 2**-24 and 1
  * act: ids up to 2**31 - 2, seed 2**64 - 1, counters 2**32 - 1, 2**32, 2**64 - 1 against the numpy spec and Philox in Python
    integers, and the split at that offset
  * act: n in {15, 16, 17, 32, 33}; 1 / 3 and 5 / 1 weight replicas with NaN behind the last; the staged rows 4, 8, 12 bytes off;
    student_out / source_out NULL; a teacher whose output is NaN
  * every refusal the header promises, at the C ABI: the code, a word of rover_last_error() where the header is specific, and no
    output touched
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dagger_helpers as H
from td3_helpers import INDEX_BATCHES, INDEX_MEM_ROWS, TOP_COUNTERS, TOP_OFFSET, TOP_SEED, same_bits_nan_aware
from test_dagger import env_rows, images
from test_gpu_dagger import biteq, net, rover_net
from test_gpu_td3_collect import SENTINEL, SPECIAL_BITS, _guarded, _guards_intact

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF, NAN = float("inf"), float("nan")


def D():
    from isaac_rover_orbit_amd import dagger
    return dagger


def guards_ok(bufs):
    return all(_guards_intact(*b) for b in bufs)


# ------------------------------------------------------------------------------------------------- 1. rows: tails, alignments
def rows_case(n, offs, rot, with_teacher=True, **hp):
    """One rover_dagger_rows launch with the four pointers ``offs`` floats off a 16-byte boundary (depth, env_raw, rows_out,
    teacher_rows_out) and rotation ``rot`` of the planted values; compares with the CPU specification."""
    h = H.hparams(**hp)
    d_buf, d, _ = _guarded(n * 961, torch.float32, offs[0])
    e_buf, e, _ = _guarded(n * 965, torch.float32, offs[1])
    d.copy_(images(n, n).reshape(-1))
    e.copy_(env_rows(n, n).reshape(-1))
    H.plant(d, e, n, SPECIAL_BITS, h.depth_clip, rot)
    out = _guarded(n * 965, torch.float32, offs[2])
    tea = _guarded(n * 965, torch.float32, offs[3])
    for t, off in zip((d, e, out[1], tea[1]), offs):
        assert t.data_ptr() % 16 == 4 * off
    H.rows(h, d, e, n, out[1], tea[1] if with_teacher else None)
    torch.cuda.synchronize()
    dc, ec = d.cpu().view(n, 961), e.cpu().view(n, 965)
    want = D().student_rows(dc, ec, float(h.depth_clip), float(h.depth_scale))
    what = (n, offs, rot, with_teacher, hp)
    assert same_bits_nan_aware(out[1].cpu().view(n, 965), want), what
    if with_teacher:
        assert biteq(tea[1].view(n, 965), D().sanitise(ec)), what
    else:
        assert bool((tea[1] == SENTINEL).all()), what
    assert guards_ok((out, tea)), what
    return out[1].cpu().view(n, 965), want


@pytest.mark.parametrize("n", [2, 3, 5])
def test_rows_tails_and_alignments(n):
    assert (n * 965) & 3 == {2: 2, 3: 3, 5: 1}[n]
    values = len(H.pixel_values(SPECIAL_BITS, 10.0))
    for rot in range(values):                                              # the vector path: every value at every place
        got, want = rows_case(n, (0, 0, 0, 0), rot)
        assert bool(torch.isfinite(got).all())
    rows_case(n, (0, 0, 0, 0), 1, with_teacher=False)                      # teacher_rows_out = NULL: still the vector path
    rot = 0
    for which in range(4):                                                 # one pointer off, the other three aligned
        for off in (1, 2, 3):
            offs = [0, 0, 0, 0]
            offs[which] = off
            rows_case(n, tuple(offs), rot % values)
            rot += 1
    for off in (1, 2, 3):                                                  # all four off together, with and without the teacher's rows
        rows_case(n, (off,) * 4, rot % values)
        rows_case(n, (off, off, off, 0), (rot + 1) % values, with_teacher=False)
        rot += 2


# ------------------------------------------------------------------------------------------------- 2. rows: hyper-parameters
@pytest.mark.parametrize("hp", [dict(depth_scale=0.0), dict(depth_scale=-0.1), dict(depth_scale=INF), dict(depth_scale=1e-45),
                                dict(depth_clip=1e-45), dict(depth_clip=H.FLT_MAX)], ids=lambda hp: "-".join(f"{k}={v}" for k, v in hp.items()))
def test_rows_hyper_parameters(hp):
    for offs in ((0, 0, 0, 0), (1, 0, 0, 0)):                              # the vector and the scalar path
        got, want = rows_case(3, offs, 2, **hp)
        pix = got[:, 4:]
        if hp.get("depth_scale") == INF:
            assert bool(torch.isnan(want[:, 4:]).any()) and bool(torch.isnan(pix).any()) and bool(torch.isinf(pix).any())
        else:
            assert bool(torch.isfinite(got).all())
        if hp.get("depth_scale") == 1e-45:
            assert float(pix.max()) > 0.0                                  # a denormal product is kept, not flushed to zero
        if hp.get("depth_scale") == -0.1:
            assert float(pix.max()) <= 0.0 and float(pix.min()) == H.f32(np.float32(-0.1) * np.float32(10.0))
        if hp.get("depth_clip") == H.FLT_MAX:
            assert float(pix.max()) == H.f32(np.float32(0.1) * np.float32(H.FLT_MAX))


# ------------------------------------------------------------------------------------------------- 3. record: indices, bookkeeping
def record_case(n, B, mem_rows, counter):
    from isaac_rover_orbit_amd import td3_collect as TC
    from test_gpu_td3_collect import _hp
    h = H.hparams(seed=TOP_SEED)
    d, e = images(n, 3).to(DEV), env_rows(n, 3).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(n)
    rew = torch.randn(n, device=DEV, generator=g)
    term = torch.tensor([0, 1, 2, 255], dtype=torch.uint8, device=DEV).repeat(n // 4 + 1)[:n].contiguous()
    slot, tea = _guarded(n * 965, torch.float32), _guarded(n * 965, torch.float32)
    rew_o, term_o = _guarded(n, torch.float32, 1), _guarded(n, torch.uint8)
    pos, idx = _guarded(1, torch.int32), _guarded(B, torch.int64)
    H.record(h, d, e, n, slot[1], tea[1], counter, rew=rew, terminated=term, rew_out=rew_o[1], term_out=term_o[1], ring_pos_entry=pos[1],
             ring_pos_value=5, idx_out=idx[1], mem_rows=mem_rows)
    # the TD3 collector's record under the same seed, counter, batch and mem_rows: the header calls the two bit-comparable
    slot3, idx3 = _guarded(n * 965, torch.float32), _guarded(B, torch.int64)
    TC.collect_record(e, slot3[1].view(n, 965), _hp(seed_lo=0xFFFFFFFF, seed_hi=0xFFFFFFFF), counter, idx_out=idx3[1], mem_rows=mem_rows)
    torch.cuda.synchronize()
    what = (n, B, mem_rows, counter)
    got = idx[1].cpu().numpy()
    assert got.tolist() == TC.sample_indices(TOP_SEED, counter, B, mem_rows).tolist(), what
    assert torch.equal(idx[1], idx3[1]), what
    assert got.min() >= 0 and got.max() < mem_rows, what
    assert torch.equal(term_o[1], (term != 0).to(torch.uint8)) and set(term_o[1].cpu().tolist()) <= {0, 1}, what
    assert biteq(rew_o[1], rew) and int(pos[1]) == 5, what
    assert biteq(slot[1].view(n, 965), D().student_rows(d.cpu(), e.cpu())) and biteq(tea[1].view(n, 965), D().sanitise(e.cpu())), what
    assert guards_ok((slot, tea, rew_o, term_o, pos, idx, slot3, idx3)), what
    return got


@pytest.mark.parametrize("n,batches", [(1, INDEX_BATCHES), (97, (3,))])
def test_record_indices_at_the_top_of_mem_rows(n, batches):
    """n = 1 is 242 pieces: with 1023 and 1025 indices the grid is sized by the batch; n = 97 with 3: by the pieces."""
    assert max(INDEX_BATCHES) > (965 + 3) // 4 > 5
    for mem_rows in INDEX_MEM_ROWS:
        for B in batches:
            record_case(n, B, mem_rows, 2 ** 32 - 1)
    lo = record_case(n, batches[-1], 2 ** 32, 2 ** 32 - 1)
    hi = record_case(n, batches[-1], 2 ** 32, 2 ** 64 - 1)                 # the counter's high word is part of the draw
    assert lo.tolist() != hi.tolist()


def test_record_without_indices_reads_neither_batch_nor_mem_rows():
    n = 3
    h = H.hparams()
    d, e = images(n, 4).to(DEV), env_rows(n, 4).to(DEV)
    slot, pos = _guarded(n * 965, torch.float32), _guarded(1, torch.int32)
    H.record(h, d, e, n, slot[1], None, 7, ring_pos_entry=pos[1], ring_pos_value=9, idx_out=None, batch=0, mem_rows=0)
    torch.cuda.synchronize()
    assert int(pos[1]) == 9 and biteq(slot[1].view(n, 965), D().student_rows(d.cpu(), e.cpu())) and guards_ok((slot, pos))


# ------------------------------------------------------------------------------------------------- 4. act
@pytest.fixture(scope="module")
def nets():
    return rover_net(net(30)), rover_net(net(31))


@pytest.fixture(scope="module")
def data():
    """(raw env rows, depth, teacher rows, student rows) of 112 envs on the device, through the rows kernel once."""
    raw, dep = env_rows(112, 5).to(DEV), images(112, 5).to(DEV)
    tea = torch.empty(112, 965, device=DEV)
    stu = D().fused_student_rows(dep, raw, teacher_rows_out=tea)
    return raw, dep, tea, stu


def act_case(teacher, student, tea_rows, stu_rows, n, seed, offset, counter, beta, student_null=False, source_null=False):
    """One rover_dagger_act call into guarded outputs; checks the guards, student_out and label_out against the two networks and the
    rest against TorchDAggerCollector's rule with the fused networks' own outputs as its callables' results."""
    h = H.hparams(seed=seed, env_id_offset=offset)
    bufs = {k: _guarded(2 * n, torch.float32) for k in ("label", "env_act", "student")}
    bufs["source"] = _guarded(n, torch.uint8)
    o = {k: (v[1].view(n, 2) if k != "source" else v[1]) for k, v in bufs.items()}
    H.act(teacher, student, h, counter, beta, tea_rows, stu_rows, n, o["label"], o["env_act"], None if student_null else o["student"],
          None if source_null else o["source"])
    torch.cuda.synchronize()
    what = (n, seed, offset, counter, beta)
    assert guards_ok(bufs.values()), what
    label, a_s = teacher(tea_rows[:n].clone()), student(stu_rows[:n].clone())         # fresh allocations: 16-byte aligned rows
    assert same_bits_nan_aware(o["label"], label), what
    if student_null:
        assert bool((o["student"] == SENTINEL).all()), what
    else:
        assert biteq(o["student"], a_s), what
    # the specification: its draw and its mix, on the CPU
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    spec = D().TorchDAggerCollector(lambda r: label.cpu(), lambda r: a_s.cpu(), ReplayMemory(2, n, device="cpu"), seed=seed, env_id_offset=offset)
    spec.teacher_rows, spec.counter = tea_rows[:n].cpu(), counter
    want = spec.act(beta)
    assert same_bits_nan_aware(o["env_act"].cpu(), want), what
    if source_null:
        assert bool((o["source"] == 99).all()), what
    else:
        assert torch.equal(o["source"].cpu().bool(), spec.last["source"]) and set(o["source"].cpu().tolist()) <= {0, 1}, what
    return {k: v.cpu().clone() for k, v in o.items()}, spec.last["source"].numpy()


def test_act_comparison_is_strict(nets, data):
    teacher, student = nets
    raw, dep, tea, stu = data
    n, seed, offset, counter = 33, (5 << 32) | 9, 1000, 3
    u = D().mix_uniforms(seed, offset + np.arange(n), counter)
    assert u.dtype == np.float32 and len(set(u.tolist())) == n
    for k in (0, 16, 32):                                                  # one env of each workgroup
        on, after = float(u[k]), float(np.nextafter(u[k], np.float32(1.0)))
        _, src_on = act_case(teacher, student, tea, stu, n, seed, offset, counter, on)
        _, src_after = act_case(teacher, student, tea, stu, n, seed, offset, counter, after)
        assert not src_on[k] and src_after[k]                              # u_k < u_k is false: the student
        assert np.array_equal(np.delete(src_on, k), np.delete(src_after, k)) and np.array_equal(src_on, u < on)
    o, src = act_case(teacher, student, tea, stu, n, seed, offset, counter, 2.0 ** -24)     # the smallest possible draw
    assert not src.any() and biteq(o["env_act"], o["student"])
    o, src = act_case(teacher, student, tea, stu, n, seed, offset, counter, 1.0)
    assert src.all() and biteq(o["env_act"], o["label"]) and not biteq(o["label"], o["student"])


def test_act_at_the_top_of_the_ranges(nets, data):
    teacher, student = nets
    raw, dep, tea, stu = data
    n = 33
    ids = TOP_OFFSET + np.arange(n)
    assert int(ids[-1]) == 2 ** 31 - 2
    patterns = []
    for counter in TOP_COUNTERS:
        u = D().mix_uniforms(TOP_SEED, ids, counter)
        assert len(set(u.tolist())) == n and 0 < int((u < 0.5).sum()) < n          # 33 distinct draws, both sides of 0.5 present
        assert u.tolist() == H.mix_uniforms_by_hand(TOP_SEED, ids, counter)         # ... which are Philox's, in Python integers
        o, src = act_case(teacher, student, tea, stu, n, TOP_SEED, TOP_OFFSET, counter, 0.5)
        assert np.array_equal(src, u < 0.5) and np.array_equal(src, np.array(H.mix_uniforms_by_hand(TOP_SEED, ids, counter)) < 0.5)
        lo, _ = act_case(teacher, student, tea[:16].contiguous(), stu[:16].contiguous(), 16, TOP_SEED, TOP_OFFSET, counter, 0.5)
        hi, _ = act_case(teacher, student, tea[16:33].contiguous(), stu[16:33].contiguous(), 17, TOP_SEED, TOP_OFFSET + 16, counter, 0.5)
        for key in o:
            assert torch.equal(o[key].view(torch.uint8), torch.cat([lo[key], hi[key]]).view(torch.uint8)), (counter, key)
        patterns.append(src.tolist())
    assert patterns[0] != patterns[1] != patterns[2] != patterns[0]


@pytest.mark.parametrize("n", [15, 16, 17, 32, 33])
def test_act_tiles_and_null_outputs(nets, data, n):
    teacher, student = nets
    raw, dep, tea, stu = data
    args = (teacher, student, tea[:n].contiguous(), stu[:n].contiguous(), n, 77, 11, 2 ** 32 + 5, 0.5)
    full, src = act_case(*args)
    assert 0 < int(src.sum()) < n
    for kw in (dict(student_null=True), dict(source_null=True), dict(student_null=True, source_null=True)):
        part, _ = act_case(*args, **kw)
        for key in ("label", "env_act"):
            assert biteq(part[key], full[key]), (kw, key)


def test_act_number_of_weight_replicas(nets, data):
    """Seven workgroups over 1 / 3 and 5 / 1 replicas of teacher / student; one more replica-sized block of NaN follows the last."""
    from isaac_rover_orbit_amd.policy import RoverNet
    raw, dep, tea, stu = data

    def copies(src, k):
        pf = src.packed.numel() // src.n_copies
        buf = torch.full(((k + 1) * pf,), NAN, dtype=torch.float32, device=DEV)
        buf[:k * pf] = src.packed[:pf].repeat(k)
        return RoverNet.from_packed(src.desc, buf[:k * pf], k), buf, k * pf
    want, _ = act_case(*nets, tea, stu, 112, 77, 11, 4, 0.5)
    for kt, ks in ((1, 3), (5, 1)):
        (t, tbuf, tn), (s, sbuf, sn) = copies(nets[0], kt), copies(nets[1], ks)
        got, _ = act_case(t, s, tea, stu, 112, 77, 11, 4, 0.5)
        for key in want:
            assert bool(torch.isfinite(got[key].float()).all()) and torch.equal(got[key], want[key]), (kt, ks, key)
        assert bool(torch.isnan(tbuf[tn:]).all()) and bool(torch.isnan(sbuf[sn:]).all())


@pytest.mark.parametrize("n", [16, 17])
def test_act_staging_alignment(nets, data, n):
    raw, dep, tea, stu = data
    want, _ = act_case(*nets, tea[:n].contiguous(), stu[:n].contiguous(), n, 77, 11, 6, 0.5)
    for t_off, s_off in ((1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 1), (2, 2), (3, 3)):
        tb, sb = torch.zeros(n * 965 + 8, device=DEV), torch.zeros(n * 965 + 8, device=DEV)
        t_rows, s_rows = tb[t_off:t_off + n * 965].view(n, 965), sb[s_off:s_off + n * 965].view(n, 965)
        t_rows.copy_(tea[:n]); s_rows.copy_(stu[:n])
        assert t_rows.data_ptr() % 16 == 4 * t_off and s_rows.data_ptr() % 16 == 4 * s_off
        got, _ = act_case(*nets, t_rows, s_rows, n, 77, 11, 6, 0.5)
        for key in want:
            assert torch.equal(got[key], want[key]), (t_off, s_off, key)


def test_act_with_a_nan_teacher(nets, data):
    """The teacher's last bias is NaN in column 0: the label is NaN there, the env takes it where the teacher is chosen and the
    student's finite value where it is not."""
    raw, dep, tea, stu = data
    bad = rover_net(net(30, bias=(NAN, 0.25)))
    n = 33
    o, src = act_case(bad, nets[1], tea[:n].contiguous(), stu[:n].contiguous(), n, 77, 11, 8, 0.5)
    assert 0 < int(src.sum()) < n
    assert bool(torch.isnan(o["label"][:, 0]).all()) and bool(torch.isfinite(o["label"][:, 1]).all())
    chosen = torch.from_numpy(src)
    assert bool(torch.isnan(o["env_act"][chosen, 0]).all()) and biteq(o["env_act"][chosen, 1], o["label"][chosen, 1])
    assert biteq(o["env_act"][~chosen], o["student"][~chosen]) and bool(torch.isfinite(o["student"]).all())


# ------------------------------------------------------------------------------------------------- 5. refusals without a launch
def test_rows_and_record_refusals_leave_every_output_alone():
    """ROVER_ERR_INVALID (1) as include/rover_dagger.h promises it for rover_dagger_rows and rover_dagger_record, on real device
    buffers: after all of them every output still holds its sentinel."""
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    n = 16
    row_bytes = 965 * 4
    d, e = images(n, 6).to(DEV), env_rows(n, 6).to(DEV)
    out, tea = torch.full((n * 965,), SENTINEL, device=DEV), torch.full((n * 965,), SENTINEL, device=DEV)
    rew, term = torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    rew_out, term_out = torch.full((n,), SENTINEL, device=DEV), torch.full((n,), 99, dtype=torch.uint8, device=DEV)
    pos, idx = torch.full((1,), -7, dtype=torch.int32, device=DEV), torch.full((8,), -7, dtype=torch.int64, device=DEV)
    # outputs that overlap an input or each other by one row; every pointer is valid device memory of one tensor
    both_e = torch.full(((2 * n - 1) * 965,), SENTINEL, device=DEV)
    both_d = torch.full(((n - 1) * 961 + n * 965,), SENTINEL, device=DEV)
    both_o = torch.full(((2 * n - 1) * 965,), SENTINEL, device=DEV)
    good = dict(hp=H.hparams(), d=d.data_ptr(), e=e.data_ptr(), n=n, out=out.data_ptr(), tea=tea.data_ptr(), rew=rew.data_ptr(),
                term=term.data_ptr(), rew_out=rew_out.data_ptr(), term_out=term_out.data_ptr(), idx=idx.data_ptr(), batch=8, rows=64)

    def rec(**kw):
        a = dict(good, **kw)
        return lib.rover_dagger_record(C.byref(a["hp"]), a["d"], a["e"], a["n"], a["out"], a["tea"], a["rew"], a["term"], a["rew_out"],
                                       a["term_out"], pos.data_ptr(), 3, a["idx"], a["batch"], a["rows"], C.c_uint64(0), None)

    def rows(**kw):
        a = dict(good, **kw)
        return lib.rover_dagger_rows(C.byref(a["hp"]), a["d"], a["e"], a["n"], a["out"], a["tea"], None)
    for call in (rows, rec):
        assert call(n=0) == 1
        for clip in (0.0, -1.0, INF, NAN):
            assert call(hp=H.hparams(depth_clip=clip)) == 1 and b"depth_clip" in lib.rover_last_error(), clip
        assert call(hp=H.hparams(depth_scale=NAN)) == 1 and b"depth_scale" in lib.rover_last_error()
        for name, kw in (("rows_out over env_raw", dict(e=both_e.data_ptr(), out=both_e.data_ptr() + (n - 1) * row_bytes)),
                         ("rows_out over depth", dict(d=both_d.data_ptr(), out=both_d.data_ptr() + (n - 1) * 961 * 4)),
                         ("teacher over env_raw", dict(e=both_e.data_ptr(), tea=both_e.data_ptr() + (n - 1) * row_bytes)),
                         ("teacher over depth", dict(d=both_d.data_ptr(), tea=both_d.data_ptr() + (n - 1) * 961 * 4)),
                         ("teacher over rows_out", dict(out=both_o.data_ptr(), tea=both_o.data_ptr() + (n - 1) * row_bytes)),
                         ("rows_out over teacher", dict(tea=both_o.data_ptr(), out=both_o.data_ptr() + (n - 1) * row_bytes))):
            assert call(**kw) == 1 and b"alias" in lib.rover_last_error(), name
    for missing in ("rew", "term", "rew_out", "term_out"):
        assert rec(**{missing: None}) == 1, missing
    assert rec(batch=0) == 1 and b"batch" in lib.rover_last_error()
    assert rec(rows=0) == 1 and b"mem_rows" in lib.rover_last_error()
    assert rec(rows=2 ** 32 + 1) == 1 and b"mem_rows" in lib.rover_last_error()
    torch.cuda.synchronize()
    for name, t in (("out", out), ("tea", tea), ("both_e", both_e), ("both_d", both_d), ("both_o", both_o), ("rew_out", rew_out)):
        assert bool((t == SENTINEL).all()), name
    assert bool((term_out == 99).all()) and int(pos) == -7 and bool((idx == -7).all())
    assert rows() == 0                                                     # and the good call of each is accepted
    torch.cuda.synchronize()
    want = D().student_rows(d.cpu(), e.cpu())
    assert biteq(out.view(n, 965), want) and int(pos) == -7
    out.fill_(SENTINEL)
    assert rec() == 0
    torch.cuda.synchronize()
    assert biteq(out.view(n, 965), want) and int(pos) == 3 and int(idx.min()) >= 0 and int(idx.max()) < 64
    assert rec(idx=None, batch=0, rows=0) == 0                             # without idx_out, batch and mem_rows are not read
    torch.cuda.synchronize()


def test_act_refusals_leave_every_output_alone(nets, data):
    from isaac_rover_orbit_amd import _lib
    from test_gpu_td3_collect import _actor
    lib = _lib.load()
    teacher, student = nets
    raw, dep, tea, stu = data
    n = 16
    outs = {k: torch.full((2 * n + 8,), SENTINEL, device=DEV) for k in ("label", "env_act", "student")}
    source = torch.full((n + 8,), 99, dtype=torch.uint8, device=DEV)
    plain = _actor(2)                                                      # the reference architecture without the tanh
    wide = _lib.PolicyDesc.from_buffer_copy(teacher.desc)
    wide.layers[5].N = 17
    hp = H.hparams()
    good = dict(t=C.byref(teacher.desc), tp=teacher.packed.data_ptr(), s=C.byref(student.desc), sp=student.packed.data_ptr(), beta=0.5, n=n,
                label=outs["label"].data_ptr(), env_act=outs["env_act"].data_ptr())

    def act(**kw):
        a = dict(good, **kw)
        return lib.rover_dagger_act(a["t"], a["tp"], teacher.n_copies, a["s"], a["sp"], student.n_copies, C.byref(hp), C.c_uint64(0),
                                    C.c_float(a["beta"]), tea.data_ptr(), stu.data_ptr(), a["n"], a["label"], a["env_act"],
                                    outs["student"].data_ptr(), source.data_ptr(), None)
    for beta in (-1e-9, float(np.nextafter(np.float32(1.0), np.float32(2.0))), NAN):
        assert act(beta=beta) == 1 and b"beta" in lib.rover_last_error(), beta
    assert act(n=0) == 1
    assert act(tp=teacher.packed.data_ptr() + 4) == 1 and b"aligned" in lib.rover_last_error()
    assert act(sp=student.packed.data_ptr() + 4) == 1 and b"aligned" in lib.rover_last_error()
    for who in ("t", "s"):
        assert act(**{who: C.byref(wide)}) == 4, who
        assert act(**{who: C.byref(plain.desc), who + "p": plain.packed.data_ptr()}) == 4, who
    assert act(env_act=outs["label"].data_ptr()) == 1 and b"alias" in lib.rover_last_error()
    assert act(env_act=outs["label"].data_ptr() + (2 * n - 1) * 4) == 1 and b"alias" in lib.rover_last_error()
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == SENTINEL).all()), k
    assert bool((source == 99).all())
    assert act() == 0
    torch.cuda.synchronize()
    assert biteq(outs["label"][:2 * n].view(n, 2), teacher(tea[:n].contiguous()))
    assert biteq(outs["student"][:2 * n].view(n, 2), student(stu[:n].contiguous()))
    assert bool((outs["label"][2 * n:] == SENTINEL).all()) and bool((source[n:] == 99).all()) and set(source[:n].cpu().tolist()) <= {0, 1}


def test_update_refusals_leave_every_output_alone():
    """rover_dagger_update's promises, one argument moved at a time: nothing is launched, so the trainer's vectors, its state and
    dz_out are what they were."""
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd.td3 import critic_desc
    from test_gpu_dagger import setup
    lib = _lib.load()
    mem, fused, _ = setup(seed=9)
    n = 48
    idx = mem.sample_indices(n, torch.Generator(device=DEV).manual_seed(1))
    dz = torch.full((2 * n + 8,), SENTINEL, device=DEV)
    fused.grad.fill_(SENTINEL); fused.adam_m.fill_(SENTINEL); fused.adam_v.fill_(SENTINEL)
    good = H.update_args(fused, mem, idx, dz_out=dz)
    assert good["ws_bytes"] == lib.rover_dagger_workspace_bytes(n) and good["valid_rows"] == (mem.slots - 1) * mem.num_envs
    keep = {k: getattr(fused, k).clone() for k in ("params", "grad", "adam_m", "adam_v", "state", "rep_a")}
    critic = critic_desc()

    def upd(**kw):
        return H.update_call(fused, dict(good, **kw))

    def moved(**kw):
        hp = _lib.DaggerHparams.from_buffer_copy(fused.hp)
        for k, v in kw.items():
            setattr(hp, k, v)
        return hp
    assert upd(n=0) == 1
    assert upd(slots=1) == 1 and b"slots" in lib.rover_last_error()
    assert upd(valid_rows=0) == 1 and b"valid_rows" in lib.rover_last_error()
    assert upd(valid_rows=(mem.slots - 1) * mem.num_envs + 1) == 1 and b"valid_rows" in lib.rover_last_error()
    assert upd(ws_bytes=good["ws_bytes"] - 1) == 1 and b"workspace" in lib.rover_last_error()
    assert upd(params=good["params"] + 4) == 1 and b"aligned" in lib.rover_last_error()
    assert upd(state=good["state"] + 4) == 1 and b"state" in lib.rover_last_error()
    assert upd(n_copies=0) == 1 and b"n_copies" in lib.rover_last_error()
    for clip in (-1.0, NAN):
        hp = moved(grad_norm_clip=clip)
        assert upd(hp=C.byref(hp)) == 1 and b"grad_norm_clip" in lib.rover_last_error(), clip
    assert upd(student=C.byref(critic)) == 4
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert biteq(getattr(fused, k).view(torch.int32), v.view(torch.int32)), k
    assert bool((dz == SENTINEL).all())
    assert upd() == 0                                                      # and the good call is accepted
    torch.cuda.synchronize()
    st = fused.stats()
    assert st["steps"] == 1 and st["bad_index"] == 0 and bool(torch.isfinite(dz[:2 * n]).all()) and bool((dz[2 * n:] == SENTINEL).all())
    a = fused.n_a                                                          # behind the network's floats the vectors are padding
    assert not bool((fused.grad[:a] == SENTINEL).any()) and not bool((fused.adam_m[:a] == SENTINEL).any())


def test_sizes_of_what_is_not_a_student():
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd.td3 import critic_desc
    from test_gpu_td3_collect import _actor
    lib = _lib.load()
    student = rover_net(net(31))
    assert lib.rover_dagger_param_floats(C.byref(student.desc)) > 0
    assert lib.rover_dagger_param_floats(C.byref(_actor(2).desc)) == 0     # no tanh
    assert lib.rover_dagger_param_floats(C.byref(critic_desc())) == 0
    assert lib.rover_dagger_workspace_bytes(0) == 0 and lib.rover_dagger_workspace_bytes(-1) == 0
    assert lib.rover_dagger_workspace_bytes(1) > 0
