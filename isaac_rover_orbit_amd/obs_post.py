"""ORBIT's observation post-processing (noise -> clip -> scale) as ONE HIP launch with counter-based draws (C ABI:
``include/rover_obs_post.h``).

The reference trains with observation corruption on (rover_env_cfg.py ``ObservationCfg.PolicyCfg.__post_init__``:
``enable_corruption = True``) and imports ORBIT's additive uniform noise for it (``rover_env_cfg.py:23``, ``Unoise``).
``RoverEnv`` finishes such terms in torch by default (``cfg.observation_post_backend = "torch"``); with ``"fused"`` the finished
row goes through ``ObsPost.apply`` instead: one launch for every term, and draws that are keyed like every other draw of this
tree -- Philox4x32-10 by the seed, addressed by (global env id, call counter, absolute column).  They do not depend on how the
envs are split over ranks and the checkpoint is the env's call counter: there is no state here.  The same kernel corrupts the
depth camera's image (``CameraCfg.noise`` / ``CameraCfg.clip``) under a tag of its own.

``TorchObsPost`` is the same interface in plain numpy on float32: the specification of the kernel (Philox restated in integer
arithmetic by ``rollout.philox4x32``, Box-Muller in float64), and it runs on the CPU.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _fused, _lib
from .rollout import philox4x32, rollout_counter, unit_uniform

ROW_TAG, DEPTH_TAG = _lib.OBS_POST_STREAM_ROW, _lib.OBS_POST_STREAM_DEPTH
LIDAR_TAG = _lib.OBS_POST_STREAM_LIDAR             # lidar frames (LidarCfg.noise / clip)
NONE, UNIFORM, GAUSSIAN, CONSTANT = _lib.OBS_POST_NONE, _lib.OBS_POST_UNIFORM, _lib.OBS_POST_GAUSSIAN, _lib.OBS_POST_CONSTANT
_MASK = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------- segments
def _f32(x) -> float:
    return C.c_float(float(x)).value


def noise_params(nz, hint: str = "") -> tuple:
    """(kind, a, b) of a noise object, read from its attributes as ``RoverEnv``'s torch path reads them: ``n_min`` / ``n_max``
    (uniform: a = n_min, b = the span as fp32 of the float64 difference), ``std`` (/ ``mean``) (gaussian) or ``bias`` (constant).
    ORBIT's ``AdditiveUniformNoiseCfg`` family carries these attributes; its ``.func`` is not called."""
    if nz is None:
        return NONE, 0.0, 0.0
    if hasattr(nz, "n_min") and hasattr(nz, "n_max"):
        return UNIFORM, float(nz.n_min), _f32(float(nz.n_max) - float(nz.n_min))
    if hasattr(nz, "std"):
        return GAUSSIAN, float(getattr(nz, "mean", 0.0)), float(nz.std)
    if hasattr(nz, "bias"):
        return CONSTANT, float(nz.bias), 0.0
    raise ValueError(f"noise {nz!r} has none of n_min / n_max, mean / std, bias: the fused kernel cannot run it{hint}")


def segment(col_lo: int, col_hi: int, noise=None, clip=None, scale: float = 1.0, what: str = "segment",
            hint: str = "") -> "_lib.ObsPostSegment":
    """One ``rover_obs_post_segment``, checked as the library checks it (the values as the fp32 struct holds them)."""
    kind, a, b = noise_params(noise, hint)
    s = _lib.ObsPostSegment()
    s.col_lo, s.col_hi, s.noise, s.a, s.b, s.scale = int(col_lo), int(col_hi), kind, a, b, float(scale)
    if clip is not None:
        if len(tuple(clip)) != 2:
            raise ValueError(f"{what}: clip must be (min, max)")
        s.has_clip, s.clip_lo, s.clip_hi = 1, float(clip[0]), float(clip[1])
        if not (math.isfinite(s.clip_lo) and math.isfinite(s.clip_hi) and s.clip_lo <= s.clip_hi):
            raise ValueError(f"{what}: clip must be finite with min <= max")
    if not all(math.isfinite(v) for v in (s.a, s.b, s.scale)):
        raise ValueError(f"{what}: noise parameters and scale must be finite")
    if kind in (UNIFORM, GAUSSIAN) and s.b < 0.0:
        raise ValueError(f"{what}: " + ("n_max must be >= n_min" if kind == UNIFORM else "std must be >= 0"))
    return s


def segments(cfg) -> list:
    """``cfg.observation_post()`` as the segment list of the observation row: actions 0..2, distance 2, heading 3, height scan
    ``4 .. 4 + num_rays``.  Empty for the stock table."""
    nx, ny = cfg.height_scanner.grid
    cols = {"actions": (0, 2), "distance": (2, 3), "heading": (3, 4), "height_scan": (4, 4 + nx * ny)}
    hint = "; observation_post_backend = 'torch' calls its .func"
    return [segment(*cols[name], noise=t.noise, clip=t.clip, scale=t.scale, what=f"observation term '{name}'", hint=hint)
            for name, t in cfg.observation_post().items()]


def image_segments(camera) -> list:
    """``CameraCfg.noise`` / ``CameraCfg.clip`` as one segment over the ``height * width`` pixels; empty when both are None."""
    if camera.noise is None and camera.clip is None:
        return []
    return [segment(0, int(camera.height) * int(camera.width), noise=camera.noise, clip=camera.clip, what="camera")]


def lidar_segments(lidar) -> list:
    """``LidarCfg.noise`` / ``LidarCfg.clip`` as one segment over the frame's rays; empty when both are None."""
    if lidar.noise is None and lidar.clip is None:
        return []
    return [segment(0, int(lidar.rays), noise=lidar.noise, clip=lidar.clip, what="lidar")]


# ------------------------------------------------------------------------------------------------------------------ the draws (spec)
def draw_words(seed: int, env_ids, counter: int, width: int, tag: int) -> np.ndarray:
    """The Philox words (len(env_ids), 4 * ceil(width / 4)) uint64: column ``c`` holds word ``c % 4`` of quad ``c // 4``."""
    ids = np.asarray(env_ids, dtype=np.uint64).reshape(-1, 1)
    quads = np.arange((width + 3) // 4, dtype=np.uint64).reshape(1, -1)
    w = philox4x32(*rollout_counter(ids, counter, quads, tag), int(seed) & _MASK, (int(seed) >> 32) & _MASK)
    return np.stack(w, axis=-1).reshape(ids.shape[0], -1)


def uniforms(seed: int, env_ids, counter: int, width: int, tag: int) -> np.ndarray:
    """u (len(env_ids), width) float32 inside (0, 1), exact."""
    return unit_uniform(draw_words(seed, env_ids, counter, width, tag))[:, :width].astype(np.float32)


def normals(seed: int, env_ids, counter: int, width: int, tag: int) -> np.ndarray:
    """e (len(env_ids), width) float64: Box-Muller on the exact uniforms in ``rollout.standard_normals``' form; words (0, 1) of a
    quad give its columns 0 (cosine) and 1 (sine), words (2, 3) its columns 2 and 3."""
    w = draw_words(seed, env_ids, counter, width, tag)
    u1, u2 = unit_uniform(w[:, 0::2]), unit_uniform(w[:, 1::2])
    rho = np.sqrt(-2.0 * np.log(u1))
    e = np.stack([rho * np.cos(2.0 * np.pi * u2), rho * np.sin(2.0 * np.pi * u2)], axis=-1).reshape(w.shape[0], -1)
    return e[:, :width]


# ------------------------------------------------------------------------------------------------------------------- the two classes
def _clip_ordered(v: np.ndarray, lo, hi) -> np.ndarray:
    """The header's clip: min(max(v, lo), hi) with -0 < +0 (IEEE 754-2019 maximum / minimum), so a tie of zeros does not depend on
    the order of the operands; every comparison with a NaN is false, so a NaN stays."""
    v = np.where((v < lo) | ((v == lo) & np.signbit(v) & ~np.signbit(lo)), lo, v)
    return np.where((v > hi) | ((v == hi) & ~np.signbit(v) & np.signbit(hi)), hi, v)


class _ObsPostBase:
    def __init__(self, segs, width: int, seed: int = 0, env_id_offset: int = 0, tag: int = ROW_TAG):
        self.segments = list(segs)
        self.width, self.seed, self.env_id_offset, self.tag = int(width), int(seed), int(env_id_offset), int(tag)
        if not 1 <= len(self.segments) <= _lib.OBS_POST_MAX_SEGMENTS:
            raise ValueError(f"between 1 and {_lib.OBS_POST_MAX_SEGMENTS} segments")
        if not 1 <= self.width <= _lib.OBS_POST_MAX_WIDTH:
            raise ValueError(f"width must be in [1, {_lib.OBS_POST_MAX_WIDTH}]")
        if self.tag & 0xFFFF:
            raise ValueError("the low 16 bits of tag must be clear")
        taken = np.zeros(self.width, dtype=bool)
        for s in self.segments:
            if not 0 <= s.col_lo < s.col_hi <= self.width:
                raise ValueError(f"segment [{s.col_lo}, {s.col_hi}) is empty or leaves the row of {self.width} columns")
            if taken[s.col_lo:s.col_hi].any():
                raise ValueError("segments overlap")
            taken[s.col_lo:s.col_hi] = True


class TorchObsPost(_ObsPostBase):
    """The CPU specification of ``ObsPost``: ``apply`` works in place on a float32 numpy array or CPU torch tensor ``(n, width)``,
    every operation one float32 operation in the kernel's order; ``apply64`` returns the float64 evaluation (the reference of the
    Gaussian columns, whose device Box-Muller is fp32)."""

    def _run(self, x: np.ndarray, counter: int, f64: bool) -> np.ndarray:
        n = x.shape[0]
        ids = self.env_id_offset + np.arange(n, dtype=np.int64)
        ft = np.float64 if f64 else np.float32
        out = x.astype(ft)
        u = e = None
        with np.errstate(invalid="ignore", over="ignore"):
            for s in self.segments:
                sl = slice(s.col_lo, s.col_hi)
                v = out[:, sl]
                a, b = ft(s.a), ft(s.b)
                if s.noise == UNIFORM:
                    if u is None:
                        u = uniforms(self.seed, ids, counter, self.width, self.tag)
                    v = (v + u[:, sl].astype(ft) * b) + a
                elif s.noise == GAUSSIAN:
                    if e is None:
                        e = normals(self.seed, ids, counter, self.width, self.tag)
                    v = (v + a) + b * e[:, sl].astype(ft)
                elif s.noise == CONSTANT:
                    v = v + a
                if s.has_clip:
                    v = _clip_ordered(v, ft(s.clip_lo), ft(s.clip_hi))               # NaN stays NaN, as torch.clip
                if s.scale != 1.0:
                    v = v * ft(s.scale)
                out[:, sl] = v
        return out

    def apply(self, rows, counter: int):
        x = rows.numpy() if isinstance(rows, torch.Tensor) else rows
        if x.dtype != np.float32 or x.ndim != 2 or x.shape[1] != self.width:
            raise ValueError(f"rows must be float32 (n, {self.width})")
        res = self._run(x, counter, False)
        for s in self.segments:            # columns outside every segment keep their bits (NaN payloads too)
            x[:, s.col_lo:s.col_hi] = res[:, s.col_lo:s.col_hi]
        return rows

    def apply64(self, rows, counter: int) -> np.ndarray:
        x = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
        return self._run(x.astype(np.float32), counter, True)


class ObsPost(_ObsPostBase):
    """The device class: ``apply(rows, counter)`` is one asynchronous ``rover_obs_post_apply`` launch on the current stream, in
    place.  ``rows``: a float32 cuda tensor, either ``(n, width)`` with unit column stride (any row pitch >= width) or contiguous
    ``(n, ...)`` with ``width`` values per row (an image).  ``seed`` and ``env_id_offset`` are plain attributes."""

    def __init__(self, segs, width: int, seed: int = 0, env_id_offset: int = 0, tag: int = ROW_TAG):
        super().__init__(segs, width, seed, env_id_offset, tag)
        _fused.require_gpu("ObsPost", "TorchObsPost is the CPU specification")
        self._lib = _lib.load()
        self._segs = (_lib.ObsPostSegment * len(self.segments))(*self.segments)

    def apply(self, rows: torch.Tensor, counter: int) -> torch.Tensor:
        pitch = _fused.row_pitch("rows", rows, self.width)
        _fused.launch("rover_obs_post_apply", rows.device, self._segs, len(self.segments), rows.data_ptr(), self.width, pitch,
                      int(rows.shape[0]), self.seed & 0xFFFFFFFFFFFFFFFF, self.env_id_offset, int(counter), self.tag)
        return rows
