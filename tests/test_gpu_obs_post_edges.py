"""The observation post-processing kernel (include/rover_obs_post.h, isaac_rover_orbit_amd.obs_post) on the MI355X where
tests/test_gpu_obs_post.py does not reach: launches that start at a quad other than 0, noisy segments that start and end inside a
quad, several noise kinds in one quad, uncovered quads in the middle of a launch, eight unsorted segments, the last quad of the widest
row, the second trip of the grid-stride loop, env ids across 2**32, zeros of both signs on a clip bound of either sign, denormals
and a side stream.  The tables are tests/obs_post_cases.py's, shared with the CPU tests of the specification (tests/test_obs_post.py).

Rules, as in tests/test_gpu_obs_post.py: uniform, constant, clip-only and uncovered columns are BIT-EQUAL to TorchObsPost.apply (every
uncovered column holds a NaN with a payload of its own, so "neither read nor written" is checked on the bits); Gaussian columns meet
|fused - spec64| <= std * B + 2 ulp(max(|x + mean|, |std * e|)) with that file's B.  Inputs are 0.2 * standard normal.
"""
import numpy as np
import pytest
import torch

from obs_post_cases import (CUT_UNCOVERED, CUT_WIDTH, SCAN_WIDTH, WIDE_WIDTH, ZERO_CLIPS, ZERO_SCALES, ZERO_X, Bias, Unoise, biteq,
                            cut, cut_rows, gaussian_columns, payload_nans, scan_only, wide, zero_row, zero_segments, zero_want)
from test_gpu_obs_post import B, COUNTER, OFFSET, SEED

pytestmark = pytest.mark.gpu

FLT_MIN = float(np.finfo(np.float32).tiny)
SENTINEL_BITS = 0x7FC0BEEF                       # a quiet NaN no kernel of this library produces
GIB = 1 << 30


def _sentinel(shape) -> torch.Tensor:
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def _check(got, x, segs, width, offset, counter, what, seed=SEED, tag=None):
    """``got`` (the kernel's rows) against the specification on the host rows ``x``: bit equality outside the Gaussian columns,
    the Gaussian bound inside; prints the Gaussian maxima."""
    from isaac_rover_orbit_amd import obs_post
    from isaac_rover_orbit_amd.obs_post import TorchObsPost
    tag = obs_post.ROW_TAG if tag is None else tag
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    n = x.shape[0]
    spec = TorchObsPost(segs, width, seed=seed, env_id_offset=offset, tag=tag)
    want = spec.apply(x.copy(), counter)
    gauss = gaussian_columns(segs)
    rest = [c for c in range(width) if c not in set(gauss)]
    assert got.shape == want.shape
    bad = np.argwhere(got[:, rest].view(np.int32) != want[:, rest].view(np.int32))
    assert bad.size == 0, f"{what}: (row, column) {[(int(r), rest[int(c)]) for r, c in bad[:8]]} differ from the specification"
    if not gauss:
        return
    spec64 = spec.apply64(x, counter)
    e = obs_post.normals(seed, (offset + np.arange(n)) % 2 ** 32, counter, width, tag)
    for s in segs:
        if s.noise != obs_post.GAUSSIAN:
            continue
        sl = slice(s.col_lo, s.col_hi)
        xm, se = np.abs(x[:, sl].astype(np.float64) + s.a), np.abs(s.b * e[:, sl])
        ulp = np.spacing(np.maximum(xm, se).astype(np.float32)).astype(np.float64)
        err = np.abs(got[:, sl].astype(np.float64) - spec64[:, sl])
        print(f"{what} n={n} cols [{s.col_lo}, {s.col_hi}): max |fused - spec64| = {err.max():.3e}, std * B = {s.b * B:.3e}, "
              f"max (err - 2 ulp) / std = {(np.maximum(err - 2 * ulp, 0.0) / s.b).max():.3e} (B = {B:.3e})")
        assert (err <= s.b * B + 2 * ulp).all(), (what, s.col_lo, s.col_hi)


# ------------------------------------------------------------------------------------------------------------------ CUT
def test_cut_table_bit_equal_and_gaussian_bound():
    """CUT (q0 = 1, eight unsorted segments, shared quads, bare quads inside the launch) at n in {1, 5, 17}: contiguous, where the
    pitch of 61 floats moves the 16-byte phase from row to row, and inside an (n, 80) buffer that starts 0, 4, 8 and 12 bytes off a
    16-byte boundary, whose padding and lead keep their bits.

    Measured on the MI355X over these launches: the largest |fused - spec64| is 1.815e-07 at std 1 ([6, 7), n = 17), 5.270e-08 at
    std 0.3 and 1.595e-08 at std 0.05; the largest max(|fused - spec64| - 2 ulp, 0) / std is 4.554e-09, against B = 2.047e-06."""
    from isaac_rover_orbit_amd.obs_post import ObsPost
    segs, width, pitch = cut(), CUT_WIDTH, 80
    post = ObsPost(segs, width, seed=SEED, env_id_offset=OFFSET)
    for n in (1, 5, 17):
        x = cut_rows(n)
        dev = torch.from_numpy(x.copy()).cuda()
        assert post.apply(dev, COUNTER) is dev
        _check(dev, x, segs, width, OFFSET, COUNTER, "contiguous")
        un = list(CUT_UNCOVERED)
        assert biteq(dev[:, un], x[:, un]) and not biteq(dev[:, 5:11], x[:, 5:11])
        for lead in (0, 1, 2, 3):
            flat = _sentinel((lead + n * pitch,))
            buf = flat[lead:].view(n, pitch)
            assert buf.data_ptr() % 16 == 4 * lead
            buf[:, :width] = torch.from_numpy(x.copy()).cuda()
            before = flat.clone()
            post.apply(buf[:, :width], COUNTER)
            _check(buf[:, :width], x, segs, width, OFFSET, COUNTER, f"pitch 80 lead {lead}")
            assert biteq(buf[:, width:], before[lead:].view(n, pitch)[:, width:]) and biteq(flat[:lead], before[:lead])


def test_draws_do_not_depend_on_the_cut():
    """uniform(0, 1) on zeros writes the uniforms themselves: one segment, eight segments and a launch that starts at quad 1 give the
    same bits in the same absolute columns."""
    from isaac_rover_orbit_amd import obs_post
    from isaac_rover_orbit_amd.obs_post import ObsPost, segment
    n, width = 5, CUT_WIDTH
    u = obs_post.uniforms(SEED, OFFSET + np.arange(n), COUNTER, width, obs_post.ROW_TAG)
    u01 = Unoise(0.0, 1.0)
    one = ObsPost([segment(0, width, noise=u01)], width, seed=SEED, env_id_offset=OFFSET).apply(torch.zeros(n, width, device="cuda"), COUNTER)
    assert biteq(one, u)
    edges = (0, 1, 2, 7, 8, 30, 31, 59, 61)
    eight = ObsPost([segment(lo, hi, noise=u01) for lo, hi in zip(edges[:-1], edges[1:])], width, seed=SEED, env_id_offset=OFFSET)
    assert len(eight.segments) == 8 and biteq(eight.apply(torch.zeros(n, width, device="cuda"), COUNTER), u)
    rows = np.zeros((n, width), np.float32)
    rows[:, :4] = payload_nans(n, range(4))
    tail = ObsPost([segment(4, width, noise=u01)], width, seed=SEED, env_id_offset=OFFSET).apply(torch.from_numpy(rows.copy()).cuda(), COUNTER)
    assert biteq(tail[:, 4:], u[:, 4:]) and biteq(tail[:, :4], rows[:, :4])


def test_scan_only_table_at_the_env_width():
    """Noise on the height scan alone, [4, 965): the launch starts at quad 1, columns 0 .. 3 are neither read nor written."""
    from isaac_rover_orbit_amd.obs_post import ObsPost
    n, width = 3, SCAN_WIDTH
    x = (0.2 * np.random.default_rng(965).standard_normal((n, width))).astype(np.float32)
    x[:, :4] = payload_nans(n, range(4))
    got = ObsPost(scan_only(), width, seed=SEED, env_id_offset=OFFSET).apply(torch.from_numpy(x.copy()).cuda(), COUNTER)
    _check(got, x, scan_only(), width, OFFSET, COUNTER, "scan only")
    assert biteq(got[:, :4], x[:, :4]) and (got.cpu().numpy()[:, 4:] != x[:, 4:]).mean() > 0.99


def test_widest_row_and_the_last_quad():
    """width = ROVER_OBS_POST_MAX_WIDTH: quad 65535 fills the low half of counter word 3.  Column 0 is the uniform of quad 0, the last
    three columns are the sine of words (0, 1) and both branches of words (2, 3) of quad 65535; nothing between is touched."""
    from isaac_rover_orbit_amd import obs_post
    from isaac_rover_orbit_amd.obs_post import ObsPost
    n, width, offset = 2, WIDE_WIDTH, 7
    ids = offset + np.arange(n)
    u = obs_post.uniforms(SEED, ids, COUNTER, width, obs_post.ROW_TAG)
    e = obs_post.normals(SEED, ids, COUNTER, width, obs_post.ROW_TAG)
    buf = _sentinel((n, width))
    buf[:, 0] = 0.0
    buf[:, width - 3:] = 0.0
    ObsPost(wide(), width, seed=SEED, env_id_offset=offset).apply(buf, COUNTER)
    assert bool((buf.view(torch.int32)[:, 1:width - 3] == SENTINEL_BITS).all())
    got = buf.cpu().numpy()
    assert biteq(got[:, 0], u[:, 0])
    want = e[:, width - 3:]                                                      # x = 0, mean = 0, std = 1: the normals themselves
    err = np.abs(got[:, width - 3:].astype(np.float64) - want)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print(f"widest row: max |fused - e64| = {err.max():.3e}, max (err - 2 ulp) = {np.maximum(err - 2 * ulp, 0.0).max():.3e} (B = {B:.3e})")
    assert (err <= B + 2 * ulp).all()
    # the same last quad, counted by hand on the integer Philox
    from isaac_rover_orbit_amd.rollout import philox4x32, rollout_counter, unit_uniform
    w = philox4x32(*rollout_counter(ids, COUNTER, 65535, obs_post.ROW_TAG), SEED & 0xFFFFFFFF, SEED >> 32)
    rho = np.sqrt(-2.0 * np.log(unit_uniform(w[2])))
    assert np.allclose(want[:, 1], rho * np.cos(2.0 * np.pi * unit_uniform(w[3])), rtol=0, atol=1e-12)


def test_env_id_wraps_at_2_32():
    """Counter word 0 is lo32(env_id_offset + r): with the offset 2**32 - 2, rows 2 .. 4 are the env ids 0 .. 2."""
    from isaac_rover_orbit_amd.obs_post import ObsPost
    n, width, segs = 5, CUT_WIDTH, cut()
    x = cut_rows(n)
    high = ObsPost(segs, width, seed=SEED, env_id_offset=2 ** 32 - 2).apply(torch.from_numpy(x.copy()).cuda(), COUNTER)
    zero = ObsPost(segs, width, seed=SEED, env_id_offset=0).apply(torch.from_numpy(x.copy()).cuda(), COUNTER)
    wrapped = ObsPost(segs, width, seed=SEED, env_id_offset=0).apply(torch.from_numpy(x[2:].copy()).cuda(), COUNTER)
    assert biteq(high[2:], wrapped)                                              # the same inputs under the env ids 0 .. 2
    free = [5, 6, 7, 8, 9, 10, 59, 60]                                           # the noisy columns that no clip can pin to a bound
    assert bool((high[:, free] != zero[:, free]).all()) and not biteq(high[:2, 41:58], zero[:2, 41:58])
    _check(high, x, segs, width, 2 ** 32 - 2, COUNTER, "offset 2**32 - 2")
    _check(zero, x, segs, width, 0, COUNTER, "offset 0")


def test_second_trip_of_the_grid_stride_loop():
    """The launch is capped at 2**20 workgroups of 256 threads; n = 4097 rows of 65536 quads are 2**28 + 65536 threads of work, so
    row 4096 is served wholly by the second trip of `t += stride`.  4.3 GB of rows is the least at which a second trip exists: the
    pitch is at least the width, so a thread of work stands for at least 16 bytes.  Only the two covered columns are computed on the
    host.  (The 64-bit division branch, total > 2**32 - 1, would need more than 64 GB of rows and is not run.)"""
    from isaac_rover_orbit_amd import obs_post
    from isaac_rover_orbit_amd.obs_post import ObsPost, segment
    from isaac_rover_orbit_amd.rollout import philox4x32, rollout_counter, unit_uniform
    free = torch.cuda.mem_get_info()[0]
    if free < 8 * GIB:
        pytest.skip(f"{free / GIB:.1f} GiB of device memory free: the second trip needs 4.3 GB of rows and 1.1 GB for the check")
    n, width = 4097, WIDE_WIDTH
    u01 = Unoise(0.0, 1.0)
    post = ObsPost([segment(0, 1, noise=u01), segment(width - 1, width, noise=u01)], width, seed=SEED, env_id_offset=OFFSET)
    buf = _sentinel((n, width))
    buf[:, 0] = 0.0
    buf[:, width - 1] = 0.0
    post.apply(buf, COUNTER)
    ids = (OFFSET + np.arange(n)).reshape(-1, 1)
    w = philox4x32(*rollout_counter(ids, COUNTER, np.array([[0, 65535]]), obs_post.ROW_TAG), SEED & 0xFFFFFFFF, SEED >> 32)
    first, last = unit_uniform(w[0][:, 0]).astype(np.float32), unit_uniform(w[3][:, 1]).astype(np.float32)
    got_first, got_last = buf[:, 0].cpu().numpy(), buf[:, width - 1].cpu().numpy()
    assert biteq(got_first[:4096], first[:4096]) and biteq(got_last[:4096], last[:4096])          # the first trip
    assert biteq(got_first[4096:], first[4096:]) and biteq(got_last[4096:], last[4096:])          # the second
    bits = buf.view(torch.int32)
    assert int((bits != SENTINEL_BITS).sum()) == 2 * n                                            # nothing else was written


# ------------------------------------------------------------------------------------------------------------------ values
def test_signed_zeros_at_a_clip_bound():
    """x in {+0, -0} under the eight clips with a zero bound, scale 1 and scale 2, against clamp_ordered: -0 < +0, so
    clip(+0, lo = -0) = +0 and clip(-0, lo = +0) = +0, clip(+0, hi = -0) = -0.  The sign bits, bit for bit.

    Measured on the MI355X: train_math.hpp's tclamp (v_max_f32 / v_min_f32, IEEE mode) returns the rule's sign in all sixteen
    cases at either scale, so the kernel keeps it; the specification's numpy clip was what disagreed (it returned the bound on a
    tie) and orders the zeros itself now."""
    from isaac_rover_orbit_amd.obs_post import ObsPost
    for scale in ZERO_SCALES:
        for n in (1, 3):
            got = ObsPost(zero_segments(scale), 16).apply(torch.from_numpy(zero_row(n)).cuda(), 0).cpu().numpy()
            want = zero_want(scale, n)
            if n == 1:
                for i, (lo, hi) in enumerate(ZERO_CLIPS):
                    for j, xv in enumerate(ZERO_X):
                        print(f"scale {scale:g} clip({xv!r:>4}, lo={lo!r:>4}, hi={hi!r:>4}) -> device {float(got[0, 2 * i + j])!r:>4}, "
                              f"rule {float(want[0, 2 * i + j])!r:>4}")
            assert biteq(got, want), (scale, n, got, want)
    # a quad that moves as one 16-byte access and a zero bound next to ordinary values
    from isaac_rover_orbit_amd.obs_post import TorchObsPost, segment
    x = np.array([[0.0, -0.0, 0.5, -0.5, -0.0, 0.0, -3.0, 9.0]], np.float32)
    for clip in ((0.0, 4.0), (-4.0, -0.0)):
        segs = [segment(0, 8, clip=clip)]
        got = ObsPost(segs, 8).apply(torch.from_numpy(x.copy()).cuda(), 0)
        assert biteq(got, TorchObsPost(segs, 8).apply(x.copy(), 0)), clip


def test_denormals_are_kept():
    """The code object keeps fp32 denormals and numpy does too: a flushing build would lose bit equality here."""
    from isaac_rover_orbit_amd.obs_post import ObsPost, TorchObsPost, segment
    vals = np.array([1e-40, -1e-40, 1.4e-45, 1e-38, FLT_MIN / 2], np.float32)
    x = np.stack([vals, -vals])
    width = vals.size
    denormal = 0
    for kw in (dict(noise=Bias(0.0), scale=0.5), dict(noise=Unoise(0.0, 1e-39)), dict(clip=(-1e-40, 1e-40))):
        segs = [segment(0, width, **kw)]
        want = TorchObsPost(segs, width, seed=SEED, env_id_offset=OFFSET).apply(x.copy(), COUNTER)
        got = ObsPost(segs, width, seed=SEED, env_id_offset=OFFSET).apply(torch.from_numpy(x.copy()).cuda(), COUNTER)
        assert biteq(got, want), (kw, got.cpu().numpy(), want)
        here = int(((want != 0.0) & (np.abs(want) < FLT_MIN)).sum())
        assert here >= 1, kw                                                    # not vacuous: the expected values hold denormals
        denormal += here
    assert denormal >= 10


def test_apply_on_a_side_stream():
    """apply launches on the current stream: rows filled, processed and read on a side stream are the specification's while the
    default stream is busy with an unrelated fill."""
    from isaac_rover_orbit_amd.obs_post import ObsPost
    n, width, segs = 17, CUT_WIDTH, cut()
    x = cut_rows(n)
    post = ObsPost(segs, width, seed=SEED, env_id_offset=OFFSET)
    busy = torch.empty(1 << 28, device="cuda")                                   # 1 GiB: a fill of it takes a fraction of a millisecond
    src = torch.from_numpy(x.copy()).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for it in range(2):
        for _ in range(8):
            busy.fill_(float(it))
        with torch.cuda.stream(side):
            dev = torch.empty_like(src)
            dev.copy_(src)
            post.apply(dev, COUNTER + it)
            done = torch.cuda.Event()
            done.record()
            done.synchronize()
            got = dev.cpu().numpy()
        _check(got, x, segs, width, OFFSET, COUNTER + it, f"side stream, counter + {it}")
    torch.cuda.synchronize()
    assert float(busy[0]) == 1.0 and float(busy[-1]) == 1.0
