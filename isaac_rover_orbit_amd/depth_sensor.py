"""The depth camera's sensor model as ONE HIP launch with counter-based draws (C ABI: ``include/rover_depth_sensor.h``).

``rover_camera_render`` gives the exact range along each pixel's ray.  A stereo or structured-light camera has a working range,
loses pixels (mostly along occlusion edges), errs with the square of the range and reports depth in disparity steps.
``DepthSensor.apply`` puts these four effects on a batch of depth images: range -> edge-aware dropout -> axial noise ->
disparity quantisation -> fill, per pixel and in that order (the header has the sequence operation by operation).  The draws are
keyed like every other draw of this tree -- Philox4x32-10 by the seed, addressed by (global env id, call counter, absolute pixel)
under two tags of their own -- so they do not depend on how the envs are split over ranks, and the checkpoint is the env's call
counter: there is no state here.  ``RoverEnv`` runs it behind the render when ``cfg.camera.sensor`` is set, ahead of
``CameraCfg.noise`` / ``CameraCfg.clip``.

``TorchDepthSensor`` is the same interface in plain numpy on float32: the specification of the kernel (Philox restated in integer
arithmetic by ``rollout.philox4x32``, the normals as ``obs_post.normals`` forms them: Box-Muller in float64), and it runs on the
CPU.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _fused, _lib
from .obs_post import normals, uniforms

NORMAL_TAG, DROPOUT_TAG = _lib.DEPTH_SENSOR_STREAM_NORMAL, _lib.DEPTH_SENSOR_STREAM_DROPOUT
MAX_PIXELS = _lib.DEPTH_SENSOR_MAX_PIXELS
TAGS = {"depth_sensor_normal": NORMAL_TAG, "depth_sensor_dropout": DROPOUT_TAG}   # td3_explore.TAGS is the repository's table


def native_cfg(camera) -> "_lib.DepthSensorCfg":
    """``camera.sensor`` (a ``cfg.DepthSensorCfg``) as the library's struct, with fb from ``camera.focal_px[0]``."""
    return camera.sensor.to_native(camera.focal_px[0])


class _DepthSensorBase:
    def __init__(self, cfg: "_lib.DepthSensorCfg", height: int, width: int, seed: int = 0, env_id_offset: int = 0):
        if not isinstance(cfg, _lib.DepthSensorCfg):
            raise TypeError("cfg must be a _lib.DepthSensorCfg (cfg.DepthSensorCfg.to_native(focal_px) makes one)")
        self.cfg = cfg
        self.height, self.width = int(height), int(width)
        self.seed, self.env_id_offset = int(seed), int(env_id_offset)
        if self.height < 1 or self.width < 1:
            raise ValueError("height and width must be >= 1")
        if self.height * self.width > MAX_PIXELS:
            raise ValueError(f"height * width must be <= {MAX_PIXELS}")

    @property
    def pixels(self) -> int:
        return self.height * self.width


class TorchDepthSensor(_DepthSensorBase):
    """The CPU specification of ``DepthSensor``.  ``apply`` takes float32 numpy arrays or CPU torch tensors holding ``height *
    width`` consecutive values per image, every operation one float32 operation in the kernel's order.  With ``float64=True`` the
    noise stage's product and sum ``z + sigma(z) * e`` (and what follows them) run in float64 on the float64 normals, under the
    fp32 ``sigma(z)``, and ``apply`` returns a new float64 array: the reference of the Gaussian stage, whose device Box-Muller is
    fp32."""

    def __init__(self, cfg, height: int, width: int, seed: int = 0, env_id_offset: int = 0, float64: bool = False):
        super().__init__(cfg, height, width, seed, env_id_offset)
        self.float64 = bool(float64)

    def stages(self, images: np.ndarray, counter: int) -> dict:
        """Every stage of ``images`` (n, height * width) float32: ``in_range`` (step 1), ``edge`` (step 2, meaningful where
        in_range), ``kept`` (valid after step 3), ``noisy`` (step 4), ``dk`` (d * inv_step of step 5 evaluated in float64 on the
        stage's own noisy depth), ``k`` (step 5's integer as a float), ``valid`` and ``out``."""
        c, H, W = self.cfg, self.height, self.width
        n, hw = images.shape[0], self.pixels
        ids = self.env_id_offset + np.arange(n, dtype=np.int64)
        f32 = np.float32
        z0 = np.ascontiguousarray(images, dtype=f32).reshape(n, hw)
        with np.errstate(all="ignore"):
            in_range = (z0 >= f32(c.range_min)) & (z0 <= f32(c.range_max))
            Z, R = z0.reshape(n, H, W), in_range.reshape(n, H, W)
            E = np.zeros((n, H, W), dtype=bool)

            def to(zc, zn, rn):
                return np.where(rn, np.abs(zc - zn) > f32(c.edge_rel) * np.minimum(zc, zn), bool(c.edge_at_invalid))

            E[:, 1:, :] |= to(Z[:, 1:, :], Z[:, :-1, :], R[:, :-1, :])        # up
            E[:, :-1, :] |= to(Z[:, :-1, :], Z[:, 1:, :], R[:, 1:, :])        # down
            E[:, :, 1:] |= to(Z[:, :, 1:], Z[:, :, :-1], R[:, :, :-1])        # left: column 0 has none
            E[:, :, :-1] |= to(Z[:, :, :-1], Z[:, :, 1:], R[:, :, 1:])        # right: the last column has none
            edge = E.reshape(n, hw)
            u = uniforms(self.seed, ids, counter, hw, DROPOUT_TAG)
            kept = in_range & ~(u < np.where(edge, f32(c.p_edge), f32(c.p_drop)))
            ft = np.float64 if self.float64 else f32
            e = normals(self.seed, ids, counter, hw, NORMAL_TAG).astype(ft)
            t = z0 * f32(c.sigma2)                                            # sigma(z) is the fp32 value in both evaluations
            t = t + f32(c.sigma1)
            t = z0 * t
            s = t + f32(c.sigma0)
            noisy = z0.astype(ft) + s.astype(ft) * e
            valid, out = kept, noisy
            dk = k = np.full((n, hw), np.nan)
            if c.disparity_step > 0.0:
                dk = (np.float64(c.fb) / noisy.astype(np.float64)) * np.float64(c.inv_step)
                k = np.rint((ft(c.fb) / noisy) * ft(c.inv_step))              # ties to even
                valid = kept & (k >= 1.0)
                out = ft(c.fb) / (k * ft(c.disparity_step))
            out = np.where(valid, out, ft(c.invalid_value))
        return {"in_range": in_range, "edge": edge, "kept": kept, "noisy": noisy, "sigma": s, "dk": dk, "k": k, "valid": valid,
                "out": out}

    def apply(self, buf, counter: int, out=None, valid_out=None):
        x = buf.numpy() if isinstance(buf, torch.Tensor) else buf
        if x.dtype != np.float32 or x.ndim < 2 or x[0].size != self.pixels:
            raise ValueError(f"buf must be float32 (n, ...) with {self.pixels} values per image")
        st = self.stages(x.reshape(x.shape[0], -1), counter)
        if valid_out is not None:
            v = valid_out.numpy() if isinstance(valid_out, torch.Tensor) else valid_out
            v[...] = st["valid"].sum(axis=1).astype(np.int32)
        if self.float64:
            return st["out"].reshape(x.shape)
        dst = x if out is None else (out.numpy() if isinstance(out, torch.Tensor) else out)
        dst[...] = st["out"].reshape(x.shape)
        return buf if out is None else out


class DepthSensor(_DepthSensorBase):
    """The device class: ``apply(buf, counter, out=None, valid_out=None)`` is one asynchronous ``rover_depth_sensor_apply`` launch
    on the current stream.  ``buf``: a float32 cuda tensor, either contiguous ``(n, ...)`` with ``height * width`` values per image
    or ``(n, height * width)`` with unit column stride and any row pitch >= height * width.  ``out`` (default: in place) has
    ``buf``'s layout and pitch; ``valid_out`` is a contiguous int32 cuda tensor of ``n`` counts.  ``seed`` and ``env_id_offset`` are
    plain attributes."""

    def __init__(self, cfg, height: int, width: int, seed: int = 0, env_id_offset: int = 0):
        super().__init__(cfg, height, width, seed, env_id_offset)
        _fused.require_gpu("DepthSensor", "TorchDepthSensor is the CPU specification")
        self._lib = _lib.load()

    @classmethod
    def from_camera(cls, camera, seed: int = 0, env_id_offset: int = 0) -> "DepthSensor":
        """The sensor of a ``cfg.CameraCfg`` whose ``sensor`` is set."""
        return cls(native_cfg(camera), camera.height, camera.width, seed, env_id_offset)

    def _pitch(self, t: torch.Tensor, name: str) -> int:
        return _fused.row_pitch(name, t, self.pixels)

    def apply(self, buf: torch.Tensor, counter: int, out: torch.Tensor | None = None, valid_out: torch.Tensor | None = None):
        pitch = self._pitch(buf, "buf")
        n = int(buf.shape[0])
        if out is not None and (out.device != buf.device or out.shape[0] != n or self._pitch(out, "out") != pitch):
            raise ValueError("out must have buf's device, layout and pitch")
        if valid_out is not None and (valid_out.device != buf.device or valid_out.dtype != torch.int32 or
                                      not valid_out.is_contiguous() or valid_out.numel() != n):
            raise ValueError(f"valid_out must be a contiguous int32 cuda tensor of {n} counts on buf's device")
        dst = buf if out is None else out
        _fused.launch("rover_depth_sensor_apply", buf.device, self.cfg, buf.data_ptr(), dst.data_ptr(), self.height, self.width,
                      int(pitch), n, self.seed & 0xFFFFFFFFFFFFFFFF, self.env_id_offset, int(counter), _fused.ptr(valid_out))
        return dst
