"""What the observation post-processing edge tests share (not a test module): tests/test_obs_post.py and
tests/test_gpu_obs_post_edges.py, so that the CPU and the GPU tests stay on the same inputs.

``Unoise`` / ``Gnoise`` / ``Bias``   noise objects with the attributes ``obs_post.noise_params`` reads.
``biteq``            int32 equality of two float32 arrays or tensors (NaN payloads and the sign of a zero count).
``clamp_ordered``    the clip rule of include/rover_obs_post.h in plain Python, one element at a time: -0 < +0, a NaN stays.
``ZERO_CLIPS`` ...   the signed-zero table: every pairing of a zero input with a zero clip bound.
``cut()``            CUT: width 61, eight segments in unsorted order; noisy segments that start and end inside a quad, three noise
                     kinds in quad 1, one-column segments, a Gaussian segment that holds only the sine column of a pair, quads with
                     no segment in the middle of the launch, and column 0 uncovered (the launch starts at quad 1).
``scan_only()``      SCAN_ONLY: noise on the height scan alone at the env's width, [4, 965): the launch starts at quad 1.
``wide()``           WIDE: the widest row the ABI takes, a segment on column 0 and one on the last three columns (quad 65535).
"""
import math

import numpy as np
import torch


class Unoise:
    def __init__(self, n_min, n_max):
        self.n_min, self.n_max = n_min, n_max


class Gnoise:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std


class Bias:
    def __init__(self, bias):
        self.bias = bias


def _host(a) -> np.ndarray:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a)


def biteq(a, b) -> bool:
    a, b = _host(a), _host(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------------------------------------ the clip rule
def _key(v: float):
    """The total order of the rule on non-NaN floats: by value, and -0 before +0."""
    return (v, 0 if math.copysign(1.0, v) < 0.0 else 1)


def clamp_ordered(x: float, lo: float, hi: float) -> float:
    """min(max(x, lo), hi) under -0 < +0 (IEEE 754-2019 maximum / minimum); a NaN passes through."""
    x, lo, hi = float(x), float(lo), float(hi)
    if x != x:
        return x
    m = x if _key(x) >= _key(lo) else lo
    return m if _key(m) <= _key(hi) else hi


ZERO_X = (0.0, -0.0)
ZERO_CLIPS = ((0.0, 4.0), (-0.0, 4.0), (-4.0, 0.0), (-4.0, -0.0), (0.0, 0.0), (-0.0, -0.0), (-0.0, 0.0), (0.0, -0.0))
ZERO_SCALES = (1.0, 2.0)


def zero_segments(scale: float) -> list:
    """The eight clips of ZERO_CLIPS as eight segments of two columns each (width 16): column 2 i takes +0.0 and 2 i + 1 takes -0.0
    (``zero_row``)."""
    from isaac_rover_orbit_amd.obs_post import segment
    return [segment(2 * i, 2 * i + 2, clip=c, scale=scale) for i, c in enumerate(ZERO_CLIPS)]


def zero_row(n: int = 1) -> np.ndarray:
    return np.tile(np.array(ZERO_X, np.float32), (n, len(ZERO_CLIPS)))


def zero_want(scale: float, n: int = 1) -> np.ndarray:
    """``clamp_ordered`` on ``zero_row`` under ``zero_segments``; the scale as one float32 multiplication."""
    row = [np.float32(clamp_ordered(x, lo, hi)) for lo, hi in ZERO_CLIPS for x in ZERO_X]
    row = np.array(row, np.float32)
    if scale != 1.0:
        row = row * np.float32(scale)
    return np.tile(row, (n, 1))


# ------------------------------------------------------------------------------------------------------------------ the tables
CUT_WIDTH = 61
CUT_UNCOVERED = tuple(range(0, 5)) + tuple(range(11, 22)) + tuple(range(26, 41)) + (58,)
SCAN_WIDTH = 965
WIDE_WIDTH = 262144


def cut() -> list:
    from isaac_rover_orbit_amd.obs_post import segment
    return [segment(41, 47, noise=Gnoise(0.1, 0.3), clip=(-0.5, 0.5)),
            segment(5, 6, noise=Unoise(-1.0, 1.0)),
            segment(6, 7, noise=Gnoise(0.0, 1.0)),
            segment(7, 11, noise=Unoise(0.0, 0.5), scale=-2.0),
            segment(22, 23, noise=Bias(0.25)),
            segment(23, 26, clip=(-0.1, 0.1)),
            segment(47, 58, noise=Unoise(-0.02, 0.03), clip=(-0.25, 0.12), scale=2.0),
            segment(59, 61, noise=Gnoise(0.0, 0.05))]


def scan_only() -> list:
    from isaac_rover_orbit_amd.obs_post import segment
    return [segment(4, SCAN_WIDTH, noise=Unoise(-0.02, 0.03))]


def wide() -> list:
    from isaac_rover_orbit_amd.obs_post import segment
    return [segment(0, 1, noise=Unoise(0.0, 1.0)), segment(WIDE_WIDTH - 3, WIDE_WIDTH, noise=Gnoise(0.0, 1.0))]


def payload_nans(n: int, cols, base: int = 0x7FC01000) -> np.ndarray:
    """(n, len(cols)) float32 NaNs, each with a payload of its own: what a column no segment covers holds."""
    k = len(cols)
    return (base + np.arange(n * k, dtype=np.uint32).reshape(n, k)).view(np.float32)


def cut_rows(n: int, seed: int = 0) -> np.ndarray:
    """(n, 61) float32: 0.2 * standard normal, a payload NaN in every column CUT leaves alone."""
    x = (0.2 * np.random.default_rng(61000 + 7 * n + seed).standard_normal((n, CUT_WIDTH))).astype(np.float32)
    x[:, list(CUT_UNCOVERED)] = payload_nans(n, CUT_UNCOVERED)
    return x


def gaussian_columns(segs) -> list:
    from isaac_rover_orbit_amd import obs_post
    return [c for s in segs if s.noise == obs_post.GAUSSIAN for c in range(s.col_lo, s.col_hi)]
