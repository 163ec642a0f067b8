"""ORBIT's observation post-processing as one launch (include/rover_obs_post.h, isaac_rover_orbit_amd.obs_post): what needs no GPU.

  * segments(): the cfg tables -> the segment list (stock, the noise test's table, a 3 x 3 scanner, the compat shim's noise cfgs)
  * TorchObsPost (the CPU specification) against a hand-written loop over (row, column) on rollout.philox4x32: the draw addressing
  * normals() and the CUT table of tests/obs_post_cases.py against Python integers and math.*; the clip's order of the zeros
  * moments of the draws, shards, counters and tags
  * every refusal of rover_obs_post_apply through the library (checked before the device is looked at)
  * the kernel's scratch size from the code object
"""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from isaac_rover_orbit_amd import _lib, obs_post
from isaac_rover_orbit_amd.obs_post import DEPTH_TAG, ROW_TAG, TorchObsPost, segment, segments
from isaac_rover_orbit_amd.rollout import philox4x32, unit_uniform


class Unoise:
    def __init__(self, n_min, n_max):
        self.n_min, self.n_max = n_min, n_max


class Gnoise:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std


class Bias:
    def __init__(self, bias):
        self.bias = bias


def _fields(s):
    return (s.col_lo, s.col_hi, s.noise, s.a, s.b, s.has_clip, s.clip_lo, s.clip_hi, s.scale)


def f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------------- segments()
def test_segments_of_the_cfg_tables():
    from isaac_rover_orbit_amd.cfg import RoverEnvCfg
    assert segments(RoverEnvCfg()) == []                                      # the stock table: nothing to do
    # the table of test_gpu_user_terms.py::test_observation_noise_clip_scale_follow_orbit_order
    cfg = RoverEnvCfg()
    hs = cfg.observations["height_scan"]
    hs.noise, hs.clip, hs.scale = Unoise(-0.02, 0.03), (-0.25, 0.12), 2.0
    cfg.observations["distance"].clip = (0.0, 4.0)
    cfg.observation_post_backend = "fused"
    cfg.validate()
    d, s = segments(cfg)
    assert _fields(d) == (2, 3, obs_post.NONE, 0.0, 0.0, 1, 0.0, 4.0, f32(0.11))
    span = f32(0.03 - (-0.02))                                               # the float64 difference, rounded once: the torch path's scalar
    assert _fields(s) == (4, 965, obs_post.UNIFORM, f32(-0.02), span, 1, f32(-0.25), f32(0.12), 2.0)
    # a 3 x 3 scanner: 13 columns
    cfg = RoverEnvCfg()
    cfg.height_scanner.size, cfg.height_scanner.resolution = (0.2, 0.2), 0.1
    assert cfg.height_scanner.grid == (3, 3)
    cfg.observations["height_scan"].noise = Gnoise(0.01, 0.05)
    cfg.observations["actions"].scale = 0.5
    cfg.observations["heading"].noise = Bias(0.25)
    a, h, s = segments(cfg)
    assert _fields(a) == (0, 2, obs_post.NONE, 0.0, 0.0, 0, 0.0, 0.0, 0.5)
    assert _fields(h)[:5] == (3, 4, obs_post.CONSTANT, 0.25, 0.0)
    assert _fields(s)[:6] == (4, 13, obs_post.GAUSSIAN, f32(0.01), f32(0.05), 0)


def test_segments_read_the_compat_noise_cfgs_and_refuse_the_rest():
    from isaac_rover_orbit_amd.cfg import RoverEnvCfg
    from isaac_rover_orbit_amd.compat import orbit_shim as sh
    u, g, b = sh.AdditiveUniformNoiseCfg(n_min=-0.1, n_max=0.3), sh.AdditiveGaussianNoiseCfg(mean=0.5, std=0.25), sh.ConstantBiasNoiseCfg(bias=-2.0)
    assert obs_post.noise_params(u) == (obs_post.UNIFORM, -0.1, f32(0.3 - (-0.1)))
    assert obs_post.noise_params(g) == (obs_post.GAUSSIAN, 0.5, 0.25)
    assert obs_post.noise_params(b) == (obs_post.CONSTANT, -2.0, 0.0)
    assert obs_post.noise_params(None) == (obs_post.NONE, 0.0, 0.0)

    class Other:                                                             # an ORBIT-style cfg with a func only: torch can run it
        func = staticmethod(lambda data, cfg: data)

    cfg = RoverEnvCfg()
    cfg.observations["height_scan"].noise = Other()
    cfg.validate()                                                           # the torch backend takes it
    with pytest.raises(ValueError, match="torch"):
        segments(cfg)
    cfg.observation_post_backend = "fused"
    with pytest.raises(ValueError, match="torch"):
        cfg.validate()
    cfg.observation_post_backend = "hip"
    with pytest.raises(ValueError, match="observation_post_backend"):
        cfg.validate()
    for bad in (dict(noise=Unoise(0.1, -0.1)), dict(noise=Gnoise(0.0, -1.0)), dict(clip=(1.0, 0.0)), dict(clip=(0.0, math.inf)),
                dict(scale=math.nan), dict(noise=Bias(math.inf)), dict(clip=(0.0, 1.0, 2.0))):
        with pytest.raises(ValueError):
            segment(0, 4, **bad)


def test_camera_cfg_checks_noise_and_clip():
    from isaac_rover_orbit_amd.cfg import CameraCfg
    assert obs_post.image_segments(CameraCfg()) == []
    cam = CameraCfg(noise=Gnoise(0.0, 0.02), clip=(0.1, 12.0))
    cam.validate()
    (s,) = obs_post.image_segments(cam)
    assert _fields(s) == (0, 90 * 160, obs_post.GAUSSIAN, 0.0, f32(0.02), 1, f32(0.1), 12.0, 1.0)
    with pytest.raises(ValueError):
        CameraCfg(clip=(2.0, 1.0)).validate()
    with pytest.raises(ValueError, match="cannot run"):
        CameraCfg(noise=object()).validate()
    with pytest.raises(ValueError):
        CameraCfg(width=1024, height=512, clip=(0.0, 1.0)).validate()      # 2**19 pixels: more quads than word 3 addresses


# ------------------------------------------------------------------------------------------------- the specification's draws
def test_uniform_spec_against_a_hand_written_loop():
    """Column c of global env id g takes word c % 4 of Philox(key = seed; counter = (g, counter lo, counter hi, tag | c // 4)):
    column 4 starts quad 1, and the segments 0..2 and 2..3 share quad 0."""
    seed, counter, offset, n, width = (0x1234 << 32) | 0xABCD, (7 << 32) | 5, 1000, 3, 13
    segs = [segment(0, 2, noise=Unoise(-0.5, 0.25)), segment(2, 3, noise=Unoise(0.0, 1.0)), segment(4, 13, noise=Unoise(-0.02, 0.03))]
    x = np.random.default_rng(0).standard_normal((n, width)).astype(np.float32)
    got = x.copy()
    TorchObsPost(segs, width, seed=seed, env_id_offset=offset).apply(got, counter)
    want = x.copy()
    for r in range(n):
        for s in segs:
            for c in range(s.col_lo, s.col_hi):
                w = philox4x32(offset + r, 5, 7, ROW_TAG | (c // 4), 0xABCD, 0x1234)[c % 4]
                u = np.float32(unit_uniform(w))
                want[r, c] = (x[r, c] + u * np.float32(s.b)) + np.float32(s.a)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(got[:, 3].view(np.int32), x[:, 3].view(np.int32))                 # no segment: untouched
    # the draws do not depend on how the row is cut: one segment over 0..3 draws what the two above drew
    u_all = obs_post.uniforms(seed, offset + np.arange(n), counter, width, ROW_TAG)
    one = np.zeros((n, width), np.float32)
    TorchObsPost([segment(0, 13, noise=Unoise(0.0, 1.0))], width, seed=seed, env_id_offset=offset).apply(one, counter)
    assert np.array_equal(one, u_all)
    assert np.array_equal(got[:, 2], (x[:, 2] + u_all[:, 2] * np.float32(1.0)) + np.float32(0.0))


def _philox_by_hand(c, k):
    """Random123's Philox4x32-10 on Python integers, as td3_helpers.eps_float64_by_hand restates it: (c0, c1, c2, c3), (k0, k1) ->
    four 32-bit words."""
    F = 0xFFFFFFFF
    c, k = [int(v) & F for v in c], [int(v) & F for v in k]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & F, (p0 >> 32) ^ c[3] ^ k[1], p0 & F]
        k = [(k[0] + 0x9E3779B9) & F, (k[1] + 0xBB67AE85) & F]
    return c


def _u_by_hand(w: int) -> float:
    return ((w >> 9) + 0.5) * 2.0 ** -23


def test_gaussian_spec_against_a_hand_written_loop():
    """obs_post.normals against Python integers and math.*: words (0, 1) of quad q give columns 4 q (cosine) and 4 q + 1 (sine),
    words (2, 3) give 4 q + 2 and 4 q + 3.  13 columns: the last quad gives its cosine column alone.  Tolerance
    4 * 2**-52 * max(1, |e|): both sides are float64, the margin is for last-bit differences between libm's and numpy's log, cos
    and sin."""
    seed, counter, offset, n, width = (0x1234 << 32) | 0xABCD, (7 << 32) | 5, 1000, 3, 13
    got = obs_post.normals(seed, offset + np.arange(n), counter, width, ROW_TAG)
    assert got.shape == (n, width) and got.dtype == np.float64
    for r in range(n):
        for c in range(width):
            w = _philox_by_hand((offset + r, 5, 7, ROW_TAG | (c // 4)), (0xABCD, 0x1234))
            wa, wb = (w[0], w[1]) if c % 4 < 2 else (w[2], w[3])
            rho = math.sqrt(-2.0 * math.log(_u_by_hand(wa)))
            ang = 2.0 * math.pi * _u_by_hand(wb)
            e = rho * (math.cos(ang) if c % 2 == 0 else math.sin(ang))
            assert abs(got[r, c] - e) <= 4 * 2.0 ** -52 * max(1.0, abs(e)), (r, c, got[r, c], e)
    # the uniform and the Gaussian draws read the same words: column c's uniform is the word a hand count gives it
    u = obs_post.uniforms(seed, offset + np.arange(n), counter, width, ROW_TAG)
    w = _philox_by_hand((offset + 2, 5, 7, ROW_TAG | 3), (0xABCD, 0x1234))
    assert float(u[2, 12]) == _u_by_hand(w[0])


def test_spec_clip_orders_the_zeros():
    """The clip rule of include/rover_obs_post.h at ties of zeros: -0 < +0, whatever the order of the operands.  numpy's own
    minimum / maximum return the bound on such a tie here, and which operand a SIMD lane returns is not something to rely on, so
    the lengths cover a scalar tail, one vector and more than one."""
    from obs_post_cases import ZERO_CLIPS, ZERO_SCALES, ZERO_X, clamp_ordered, zero_row, zero_segments, zero_want
    for scale in ZERO_SCALES:
        for length in (1, 3, 8, 17):
            for (lo, hi) in ZERO_CLIPS:
                x = np.array([ZERO_X[(i + i // 3) % 2] for i in range(length)], np.float32)
                rows = np.stack([x, -x])
                want = np.array([[np.float32(clamp_ordered(v, lo, hi)) * np.float32(scale) for v in row] for row in rows], np.float32)
                got = TorchObsPost([segment(0, length, clip=(lo, hi), scale=scale)], length).apply(rows.copy(), 0)
                assert np.array_equal(got.view(np.int32), want.view(np.int32)), (scale, length, lo, hi, got, want)
                got64 = TorchObsPost([segment(0, length, clip=(lo, hi), scale=scale)], length).apply64(rows, 0)
                assert np.array_equal(np.signbit(got64), np.signbit(want)) and np.array_equal(got64, want)
        # the table as the GPU test runs it: eight segments of two columns
        got = TorchObsPost(zero_segments(scale), 16).apply(zero_row(3), 0)
        assert np.array_equal(got.view(np.int32), zero_want(scale, 3).view(np.int32))
    # what the rule says, spelled out once
    assert [math.copysign(1.0, clamp_ordered(x, lo, hi)) for x, lo, hi in
            ((0.0, -0.0, 4.0), (-0.0, 0.0, 4.0), (0.0, -4.0, -0.0), (-0.0, -4.0, 0.0), (0.0, 0.0, -0.0))] == [1.0, 1.0, -1.0, -1.0, -1.0]
    assert math.isnan(clamp_ordered(math.nan, 0.0, 0.0)) and clamp_ordered(-math.inf, -0.0, 4.0) == 0.0
    assert math.copysign(1.0, clamp_ordered(-math.inf, -0.0, 4.0)) == -1.0
    # away from ties the rule is the plain clip, NaN staying
    x = np.array([[math.nan, -1.0, 0.05, 7.0, -math.inf, math.inf, -0.0, 1e-40]], np.float32)
    got = TorchObsPost([segment(0, 8, clip=(-0.5, 0.5))], 8).apply(x.copy(), 0)
    want = np.array([[np.float32(clamp_ordered(v, -0.5, 0.5)) for v in x[0]]], np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_cut_table_spec_against_a_hand_written_loop():
    """CUT's uniform, constant and clip columns element by element: three noise kinds in quad 1, one-column segments, segments given
    out of column order, a segment across two quads.  The words come from the integer Philox above, the clip from clamp_ordered;
    columns no segment covers keep their NaN payloads."""
    from obs_post_cases import CUT_UNCOVERED, CUT_WIDTH, clamp_ordered, cut, cut_rows, gaussian_columns
    seed, counter, offset, n = (0x1234 << 32) | 0xABCD, (7 << 32) | 5, 2 ** 32 - 2, 5          # rows 2 .. 4 are env ids 0 .. 2 again
    segs = cut()
    assert [s.col_lo for s in segs] != sorted(s.col_lo for s in segs) and len(segs) == _lib.OBS_POST_MAX_SEGMENTS
    assert min(s.col_lo for s in segs) // 4 == 1
    x = cut_rows(n)
    got = TorchObsPost(segs, CUT_WIDTH, seed=seed, env_id_offset=offset).apply(x.copy(), counter)
    gauss = gaussian_columns(segs)
    assert gauss == [41, 42, 43, 44, 45, 46, 6, 59, 60]
    checked = 0
    for r in range(n):
        for s in segs:
            if s.noise == obs_post.GAUSSIAN:
                continue
            for c in range(s.col_lo, s.col_hi):
                v = x[r, c]
                if s.noise == obs_post.UNIFORM:
                    w = _philox_by_hand(((offset + r) % 2 ** 32, 5, 7, ROW_TAG | (c // 4)), (0xABCD, 0x1234))[c % 4]
                    v = (v + np.float32(_u_by_hand(w)) * np.float32(s.b)) + np.float32(s.a)
                elif s.noise == obs_post.CONSTANT:
                    v = v + np.float32(s.a)
                if s.has_clip:
                    v = np.float32(clamp_ordered(v, s.clip_lo, s.clip_hi))
                if s.scale != 1.0:
                    v = v * np.float32(s.scale)
                assert got[r, c].view(np.int32) == np.float32(v).view(np.int32), (r, c)
                checked += 1
    assert checked == n * (1 + 4 + 1 + 3 + 11)
    un = list(CUT_UNCOVERED)
    assert np.array_equal(got[:, un].view(np.int32), x[:, un].view(np.int32)) and np.isnan(x[:, un]).all()
    # the Gaussian columns moved, stay finite and respect their clip; [41, 47) is clipped to +-0.5
    assert np.isfinite(got[:, gauss]).all() and (got[:, gauss] != x[:, gauss]).all() and np.abs(got[:, 41:47]).max() <= 0.5
    # env ids wrap at 2**32 (lo32 of env_id_offset + r): rows 2 .. 4 are rows 0 .. 2 of offset 0 on the same inputs
    zero = TorchObsPost(segs, CUT_WIDTH, seed=seed, env_id_offset=0).apply(x[2:].copy(), counter)
    assert np.array_equal(got[2:].view(np.int32), zero.view(np.int32))


def test_moments_of_the_draws():
    """2**16 draws (64 rows x 1024 columns).  Tolerance: 5 standard errors, each derived from the sample size N:
    uniform on (0, 1): se(mean) = sqrt(1/12 / N), se(var) = sqrt((1/80 - 1/144) / N)   (fourth central moment 1/80);
    standard normal:   se(mean) = sqrt(1 / N),    se(var) = sqrt(2 / N)."""
    n, width = 64, 1024
    N = n * width
    assert N == 2 ** 16
    u = obs_post.uniforms(99, np.arange(n), 3, width, ROW_TAG).astype(np.float64)
    e = obs_post.normals(99, np.arange(n), 3, width, ROW_TAG)
    assert u.shape == e.shape == (n, width) and u.min() > 0.0 and u.max() < 1.0
    assert abs(u.mean() - 0.5) <= 5 * math.sqrt(1 / 12 / N)                                   # 5 standard errors
    assert abs(u.var() - 1 / 12) <= 5 * math.sqrt((1 / 80 - 1 / 144) / N)                     # 5 standard errors
    assert abs(e.mean()) <= 5 * math.sqrt(1 / N)                                              # 5 standard errors
    assert abs(e.var() - 1.0) <= 5 * math.sqrt(2 / N)                                         # 5 standard errors
    # the two branches of a pair and the two pairs of a quad are uncorrelated: se of a sample correlation is 1 / sqrt(N / 4)
    q = e.reshape(n, width // 4, 4)
    for i, j in ((0, 1), (0, 2), (1, 3), (2, 3)):
        assert abs(np.corrcoef(q[..., i].ravel(), q[..., j].ravel())[0, 1]) <= 5 / math.sqrt(N / 4)   # 5 standard errors


def _mixed(width):
    return [segment(0, 2, noise=Bias(0.125), scale=0.5), segment(2, 3, clip=(0.0, 4.0), scale=0.11),
            segment(4, width, noise=Unoise(-0.02, 0.03), clip=(-0.25, 0.12), scale=2.0)]


def test_shards_counters_and_tags():
    n, k, width, seed = 17, 5, 13, 7
    x = np.random.default_rng(1).standard_normal((n, width)).astype(np.float32)
    whole = TorchObsPost(_mixed(width), width, seed=seed).apply(x.copy(), 11)
    lo = TorchObsPost(_mixed(width), width, seed=seed, env_id_offset=0).apply(x[:k].copy(), 11)
    hi = TorchObsPost(_mixed(width), width, seed=seed, env_id_offset=k).apply(x[k:].copy(), 11)
    assert np.array_equal(np.concatenate([lo, hi]), whole)                                   # rows [0, k) and [k, n) = the whole
    again = TorchObsPost(_mixed(width), width, seed=seed).apply(x.copy(), 11)
    assert np.array_equal(again.view(np.int32), whole.view(np.int32))                        # counter c twice: the same bits
    ids = np.arange(n)
    u0, u1 = obs_post.uniforms(seed, ids, 11, width, ROW_TAG), obs_post.uniforms(seed, ids, 12, width, ROW_TAG)
    assert (u0 != u1).all()                                                                  # c + 1: every column differs
    assert (u0 != obs_post.uniforms(seed, ids, 11, width, DEPTH_TAG)).all()                  # "OP" and "OD" differ
    assert (u0 != obs_post.uniforms(seed + 1, ids, 11, width, ROW_TAG)).all()
    nxt = TorchObsPost(_mixed(width), width, seed=seed).apply(x.copy(), 12)
    inside = (whole[:, 4:] > -0.5) & (whole[:, 4:] < 0.24) & (nxt[:, 4:] > -0.5) & (nxt[:, 4:] < 0.24)   # not on a clip bound
    assert inside.sum() > 10 and (whole[:, 4:][inside] != nxt[:, 4:][inside]).all()
    assert np.array_equal(whole[:, :4], nxt[:, :4])                                          # the noiseless columns do not move
    assert ROW_TAG == 0x4F500000 and DEPTH_TAG == 0x4F440000 and ROW_TAG >> 16 != DEPTH_TAG >> 16
    # neither shares its high half (the part the quad index cannot reach) with a stream of the repository's table
    from isaac_rover_orbit_amd.td3_explore import TAGS
    assert len(TAGS) >= 9 and not {ROW_TAG >> 16, DEPTH_TAG >> 16} & {v >> 16 for v in TAGS.values()}
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rover_obs_post.h")).read()
    assert dict(re.findall(r"#define ROVER_OBS_POST_STREAM_(\w+)\s+(0x[0-9A-Fa-f]{8})u", hdr)) == {"ROW": "0x4F500000", "DEPTH": "0x4F440000"}
    # the float64 evaluation agrees with the fp32 one to rounding
    assert np.allclose(TorchObsPost(_mixed(width), width, seed=seed).apply64(x, 11), whole, rtol=1e-6, atol=1e-7)


# --------------------------------------------------------------------------------------------------------------- the library
def test_every_refusal_through_the_library():
    """rover_obs_post_apply checks its arguments before it looks at the device: ROVER_ERR_INVALID with a text, on any host."""
    lib = _lib.load()
    assert lib.rover_obs_post_segment_bytes() == C.sizeof(_lib.ObsPostSegment) == 36
    buf = np.zeros(64, np.float32)
    rows = buf.ctypes.data                                    # never read: every call below is refused

    def call(segs, n_seg=None, rows=rows, width=13, pitch=13, n=2, tag=ROW_TAG):
        arr = (_lib.ObsPostSegment * max(len(segs), 1))(*segs)
        rc = lib.rover_obs_post_apply(arr if segs is not None else None, len(segs) if n_seg is None else n_seg, rows, width, pitch, n,
                                      1, 0, 0, tag, None)
        return rc, lib.rover_last_error().decode()

    def raw(col_lo=0, col_hi=4, noise=0, a=0.0, b=0.0, has_clip=0, lo=0.0, hi=0.0, scale=1.0):
        return _lib.ObsPostSegment(col_lo, col_hi, noise, a, b, has_clip, lo, hi, scale)

    ok = raw()
    nan, inf = math.nan, math.inf
    cases = [
        (dict(segs=[ok], rows=None), "NULL"),
        (dict(segs=[ok], n=0), "n must"), (dict(segs=[ok], n=-3), "n must"),
        (dict(segs=[ok], width=0), "width"), (dict(segs=[raw(0, 4)], width=262145, pitch=262145), "width"),
        (dict(segs=[ok], pitch=12), "pitch"),
        (dict(segs=[ok], n_seg=0), "n_seg"), (dict(segs=[raw(i, i + 1) for i in range(9)]), "n_seg"),
        (dict(segs=[raw(4, 4)]), "empty"), (dict(segs=[raw(5, 4)]), "empty"),
        (dict(segs=[raw(-1, 4)]), "leaves"), (dict(segs=[raw(4, 14)]), "leaves"),
        (dict(segs=[raw(0, 4), raw(3, 6)]), "overlap"), (dict(segs=[raw(2, 9), raw(0, 13)]), "overlap"),
        (dict(segs=[raw(noise=4)]), "noise kind"), (dict(segs=[raw(noise=-1)]), "noise kind"),
        (dict(segs=[raw(noise=1, a=nan)]), "finite"), (dict(segs=[raw(noise=2, b=inf)]), "finite"),
        (dict(segs=[raw(noise=3, a=-inf)]), "finite"), (dict(segs=[raw(scale=nan)]), "finite"), (dict(segs=[raw(scale=inf)]), "finite"),
        (dict(segs=[raw(has_clip=1, lo=nan, hi=1.0)]), "finite"), (dict(segs=[raw(has_clip=1, lo=0.0, hi=inf)]), "finite"),
        (dict(segs=[raw(noise=1, b=-0.5)]), "span"), (dict(segs=[raw(noise=2, b=-0.5)]), "std"),
        (dict(segs=[raw(has_clip=1, lo=1.0, hi=0.5)]), "clip_lo"),
        (dict(segs=[ok], tag=ROW_TAG | 1), "tag"), (dict(segs=[ok], tag=0x8000), "tag"),
        (dict(segs=[ok], rows=rows + 2), "aligned"),
    ]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("rover_obs_post_apply:") and text in msg, (kw, rc, msg)
    rc = lib.rover_obs_post_apply(None, 1, rows, 13, 13, 2, 1, 0, 0, ROW_TAG, None)
    assert rc == 1 and "NULL" in lib.rover_last_error().decode()
    assert not buf.any()
    # the Python classes refuse the same shapes before any call
    for bad in (dict(segs=[], width=13), dict(segs=[raw(0, 4), raw(3, 6)], width=13), dict(segs=[raw(4, 14)], width=13),
                dict(segs=[ok], width=0), dict(segs=[ok], width=13, tag=ROW_TAG | 2)):
        with pytest.raises(ValueError):
            TorchObsPost(**bad)


def test_kernel_uses_no_scratch_and_no_lds():
    from helpers import gfx950_code_objects
    from isaac_rover_orbit_amd import build
    build.build_extension()
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("ROCm llvm tools not installed")
    seen = 0
    for blob in gfx950_code_objects(_lib.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True).stdout
        for entry in re.split(r"\n\s*- \.", notes):
            m = re.search(r"\.name:\s*\S*(obs_post_kernel)\S*", entry)
            if not m or ".private_segment_fixed_size" not in entry:
                continue
            seen += 1
            assert re.search(r"\.private_segment_fixed_size:\s*0\b", entry), "obs_post_kernel uses scratch memory"
            assert re.search(r"\.group_segment_fixed_size:\s*0\b", entry), "obs_post_kernel uses LDS"
            assert int(re.search(r"\.vgpr_count:\s*(\d+)", entry).group(1)) <= 64, "eight waves per SIMD need <= 64 VGPRs"
    assert seen == 1
