"""A scanning lidar for the rover: a table of Body-frame rays cast from each env's pose against the terrain mesh, as ONE HIP launch
(C ABI: ``include/rover_lidar.h``).

The depth camera looks forward through a 110 degree lens, so a map built from it knows nothing behind the rover and little beside
it.  A rover that maps for navigation carries a scanning range sensor; ORBIT's ``RayCaster`` offers lidar patterns for it
(``patterns.LidarPatternCfg``) next to the grid pattern of the height scanner.  ``LidarCfg`` speaks that vocabulary,
``pattern_rays`` turns it into the table, ``Lidar`` casts the table on the device and ``RoverEnv`` publishes the frame as
``extras["lidar_range"]``.  The table is the one ``rover_elevation_step`` unprojects with, so ``ElevationMapCfg.source = "lidar"``
builds the rolling elevation map from the lidar instead of the camera.

``pattern_rays`` emits the table channel-major: the device gives 64 consecutive entries to one wave, so a wave marches one ring of
equal elevation angle.

``world_rays`` is the CPU specification of the origins and directions the kernel marches (numpy float32, every operation in the
header's order, compared bit for bit through ``hits_w``); ``TorchLidar`` adds a float64 cast of those rays, so the sensor and a
map fed by it run on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _fused, _lib
from .elevation import _quat_to_mat64


# ------------------------------------------------------------------------------------------------------------------- the table
def pattern_rays(cfg, dtype=np.float32) -> np.ndarray:
    """The ``(channels * azimuths, 3)`` table of unit directions in the Body frame, ring ``c`` and azimuth ``a`` at
    ``c * azimuths + a`` (channel-major).  Elevation angles are ``linspace`` over ``vertical_fov_range`` (both ends), azimuths
    ``cfg.azimuth_angles``; a ray of elevation ``el`` and azimuth ``az`` is ``(cos el cos az, cos el sin az, sin el)`` in the
    sensor frame (x forward, y left, z up: the Body frame's convention, as ``elevation.body_rays``), turned by ``orientation``.
    Computed in float64 and rounded once; the device and the specification consume this same array."""
    el = np.deg2rad(np.linspace(float(cfg.vertical_fov_range[0]), float(cfg.vertical_fov_range[1]), int(cfg.channels)))
    az = np.deg2rad(np.asarray(cfg.azimuth_angles, dtype=np.float64))
    E, A = np.meshgrid(el, az, indexing="ij")
    d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    return np.ascontiguousarray(d @ _quat_to_mat64(cfg.orientation).T, dtype=dtype)


class _Geometry:
    """What ``elevation.ElevationMap`` reads of a camera config, for a lidar frame: ``height`` rings of ``width`` rays from
    ``position``."""

    def __init__(self, cfg):
        self.height, self.width, self.position = int(cfg.channels), int(cfg.azimuths), tuple(cfg.position)


def elevation_geometry(cfg) -> _Geometry:
    """The second argument of ``ElevationMap(map_cfg, <geometry>, scanner_cfg, n, rays=pattern_rays(cfg))``."""
    return _Geometry(cfg)


# ---------------------------------------------------------------------------------------------------------------------- the spec
def world_rays(cfg, rays, pos, quat):
    """(origins ``(n, 3)``, directions ``(n, R, 3)``) float32 in the world frame: steps 1 - 4 of include/rover_lidar.h, one float32
    operation per product and sum in the header's order -- the bits the kernel marches.  ``rays`` ``(R, 3)``, ``pos`` ``(n, 3)``,
    ``quat`` ``(n, 4)`` (w, x, y, z), taken as float32."""
    ft = np.float32
    as_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)      # noqa: E731
    r = np.ascontiguousarray(as_np(rays), dtype=ft).reshape(-1, 3)
    pos, quat = as_np(pos).astype(ft).reshape(-1, 3), as_np(quat).astype(ft).reshape(-1, 4)
    m = np.array([ft(v) for v in cfg.position], dtype=ft)
    one, two, zero = ft(1.0), ft(2.0), ft(0.0)
    with np.errstate(all="ignore"):
        w, x, y, z = (quat[:, i] for i in range(4))
        s = ((w * w + x * x) + y * y) + z * z
        inv = one / np.sqrt(s)
        w, x, y, z = w * inv, x * inv, y * inv, z * inv
        r00 = one - two * (y * y + z * z)
        if cfg.attach_yaw_only:
            b = two * (w * z + x * y)
            i2 = one / np.sqrt(r00 * r00 + b * b)
            cy, sy = r00 * i2, b * i2
            zeros, ones = np.full_like(cy, zero), np.full_like(cy, one)
            R = [[cy, -sy, zeros], [sy, cy, zeros], [zeros, zeros, ones]]
        else:
            R = [[r00, two * (x * y - w * z), two * (x * z + w * y)],
                 [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                 [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]]
        o = np.stack([pos[:, i] + ((R[i][0] * m[0] + R[i][1] * m[1]) + R[i][2] * m[2]) for i in range(3)], -1)
        d = np.stack([(R[i][0][:, None] * r[None, :, 0] + R[i][1][:, None] * r[None, :, 1]) + R[i][2][:, None] * r[None, :, 2]
                      for i in range(3)], -1)
    return o.astype(ft), d.astype(ft)


def cast64(height, res, min_x, min_y, origins, dirs, near, far) -> np.ndarray:
    """Float64: the first t in [near, far] at which each ray ``origins`` (K, 3) + t ``dirs`` (K, 3) meets the triangle mesh of the
    heightfield ``height`` (H, W), row = y, cells split along the (i, j) - (i+1, j+1) diagonal; +inf where there is none or the
    ray is not finite.  A cell walk: per cell the ray is split at the diagonal and the vertical gap ray - surface is followed from
    the side the ray started on (touching counts as above; a ray that enters its range through the terrain's highest level is
    above) to the first point on the other."""
    h = np.asarray(height, dtype=np.float64)
    H, W = h.shape
    o, d = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    K = o.shape[0]
    res, min_x, min_y = float(res), float(min_x), float(min_y)
    with np.errstate(all="ignore"):
        gox, goy, gdx, gdy = (o[:, 0] - min_x) / res, (o[:, 1] - min_y) / res, d[:, 0] / res, d[:, 1] / res
        oz, dz = o[:, 2], d[:, 2]
        zmax = float(h.max())
        t_lo, t_hi = np.full(K, float(near)), np.full(K, float(far))
        miss = ~(np.isfinite(o).all(1) & np.isfinite(d).all(1))
        for g0, gd, hi in ((gox, gdx, W - 1.0), (goy, gdy, H - 1.0)):
            par = gd == 0
            a, b = -g0 / gd, (hi - g0) / gd
            t_lo = np.where(par, t_lo, np.maximum(t_lo, np.minimum(a, b)))
            t_hi = np.where(par, t_hi, np.minimum(t_hi, np.maximum(a, b)))
            miss |= par & ~((g0 >= 0) & (g0 <= hi))
        tz = (zmax - oz) / dz
        t_hi = np.where(dz > 0, np.minimum(t_hi, tz), t_hi)
        above = (dz < 0) & (tz >= t_lo)
        t_lo = np.where(dz < 0, np.maximum(t_lo, tz), t_lo)
        miss |= ((dz == 0) & (oz > zmax)) | ~(t_lo <= t_hi)
        gox, goy, gdx, gdy, oz, dz, t_lo, t_hi = (np.where(miss, 0.0, v) for v in (gox, goy, gdx, gdy, oz, dz, t_lo, t_hi))
    out = np.full(K, np.inf)
    act = np.nonzero(~miss)[0]
    sx, sy = np.where(gdx > 0, 1, -1), np.where(gdy > 0, 1, -1)
    ix = np.clip(np.floor(gox + t_lo * gdx), 0, W - 2).astype(np.int64)
    iy = np.clip(np.floor(goy + t_lo * gdy), 0, H - 2).astype(np.int64)
    t, first = t_lo.copy(), np.ones(K, bool)
    while act.size:
        a_ = act
        x0, y0, ta = ix[a_], iy[a_], t[a_]
        with np.errstate(all="ignore"):
            tx = np.where(gdx[a_] == 0, np.inf, (x0 + (sx[a_] > 0) - gox[a_]) / gdx[a_])
            ty = np.where(gdy[a_] == 0, np.inf, (y0 + (sy[a_] > 0) - goy[a_]) / gdy[a_])
        tc = np.maximum(np.minimum(np.minimum(tx, ty), t_hi[a_]), ta)
        fx0, fy0 = gox[a_] - x0, goy[a_] - y0
        h00, h01, h10, h11 = h[y0, x0], h[y0, x0 + 1], h[y0 + 1, x0], h[y0 + 1, x0 + 1]

        def gap(tt, lower):
            ca, cb = np.where(lower, h01 - h00, h11 - h10), np.where(lower, h11 - h01, h10 - h00)
            return oz[a_] + tt * dz[a_] - (h00 + (fx0 + tt * gdx[a_]) * ca + (fy0 + tt * gdy[a_]) * cb)

        e0, de = fx0 - fy0, gdx[a_] - gdy[a_]
        ea, eb = e0 + ta * de, e0 + tc * de
        split = (ea >= 0) != (eb >= 0)
        with np.errstate(all="ignore"):
            tm = np.where(split, np.clip(-e0 / de, ta, tc), tc)
        low_a = np.where(split, eb < 0, ea + eb >= 0)
        g_a, g_m, g_n = gap(ta, low_a), gap(tm, low_a), gap(tm, ~low_a)
        g_c = np.where(split, gap(tc, ~low_a), g_m)
        above[a_] = np.where(first[a_], above[a_] | (g_a >= 0), above[a_])
        first[a_] = False
        ab = above[a_]
        crossed = lambda g: np.where(ab, g <= 0, g > 0)                                      # noqa: E731
        hit_a, hit_m = crossed(g_a), crossed(g_m)
        hit_c = split & (crossed(g_n) | crossed(g_c))
        with np.errstate(all="ignore"):
            t_m = ta + (tm - ta) * g_a / (g_a - g_m)
            t_c = np.where(crossed(g_n), tm, tm + (tc - tm) * g_n / (g_n - g_c))
        hit = hit_a | hit_m | hit_c
        out[a_[hit]] = np.where(hit_a, ta, np.where(hit_m, t_m, t_c))[hit]
        step_x = tx <= ty
        nix, niy = x0 + np.where(step_x, sx[a_], 0), y0 + np.where(step_x, 0, sy[a_])
        gone = (tc >= t_hi[a_]) | (nix < 0) | (niy < 0) | (nix > W - 2) | (niy > H - 2)
        ix[a_], iy[a_], t[a_] = nix, niy, tc
        act = a_[~hit & ~gone]
    return out


class _LidarBase:
    def __init__(self, cfg):
        self.cfg = cfg
        self.native = cfg.to_native()
        self.channels, self.azimuths, self.rays = int(cfg.channels), int(cfg.azimuths), int(cfg.rays)
        self._rays32 = pattern_rays(cfg)


class TorchLidar(_LidarBase):
    """The lidar on the CPU: ``world_rays`` (the kernel's float32 origins and directions) marched in float64 by ``cast64`` over
    the heightfield ``height`` (H, W) of resolution ``res`` whose node (0, 0) lies at (``min_x``, ``min_y``).  ``cast(pos, quat)``
    returns ``(range (n, R) float32, +inf on a miss, hits_w (n, R, 3) float32 or None)``; the ranges agree with the device's to
    the march's rounding, not to the bit."""

    def __init__(self, cfg, height, res: float, min_x: float = 0.0, min_y: float = 0.0):
        super().__init__(cfg)
        self.height = np.ascontiguousarray(height, dtype=np.float32)
        self.res, self.min_x, self.min_y = float(np.float32(res)), float(np.float32(min_x)), float(np.float32(min_y))

    def cast(self, pos, quat, hits: bool | None = None):
        o, d = world_rays(self.cfg, self._rays32, pos, quat)
        n, R = d.shape[0], d.shape[1]
        org = np.repeat(o[:, None, :], R, 1).reshape(-1, 3)
        c = self.native
        rng = cast64(self.height, self.res, self.min_x, self.min_y, org, d.reshape(-1, 3), c.near_clip, c.far_clip)
        rng = rng.reshape(n, R).astype(np.float32)
        if not (self.cfg.hits if hits is None else hits):
            return rng, None
        with np.errstate(all="ignore"):
            h = o[:, None, :] + rng[:, :, None] * d
        return rng, np.where(np.isfinite(rng)[:, :, None], h, np.float32(np.inf)).astype(np.float32)


class Lidar(_LidarBase):
    """The device class.  ``env_or_handle``: a ``RoverEnv`` (its handle, device and number of envs are taken), or a ``rover_sim``
    handle with ``num_envs`` and ``device`` given.  ``prepare()`` builds the terrain's max-height pyramid (again after every
    terrain change); with ``workspace=`` the lidar adopts a workspace that ``rover_camera_prepare`` or another lidar has prepared
    for the same handle -- one pyramid serves every sensor of a handle.  ``cast(range_out, hits_out=None)`` is one asynchronous
    ``rover_lidar_cast`` launch on the current stream: ``range_out`` a float32 cuda tensor, ``(n, R)`` with unit column stride
    and any row pitch or contiguous ``(n, channels, azimuths)``; ``hits_out`` contiguous ``(n, R, 3)``."""

    def __init__(self, cfg, env_or_handle, num_envs: int | None = None, device=None, workspace: torch.Tensor | None = None):
        super().__init__(cfg)
        _fused.require_gpu("Lidar", "TorchLidar is the CPU specification")
        self._lib = _lib.load()
        if hasattr(env_or_handle, "_h"):
            self._h, self.num_envs, self.device = env_or_handle._h, int(env_or_handle.num_envs), torch.device(env_or_handle.device)
        else:
            if num_envs is None or device is None:
                raise ValueError("a bare handle needs num_envs and device")
            self._h, self.num_envs, self.device = env_or_handle, int(num_envs), torch.device(device)
        with torch.cuda.device(self.device):
            self.table = torch.from_numpy(self._rays32).to(self.device)
        self.workspace = workspace

    def prepare(self) -> "Lidar":
        nb = int(self._lib.rover_lidar_workspace_bytes(self._h))
        if nb == 0:
            raise _lib.RoverHipError("rover_lidar_workspace_bytes: no terrain bound")
        if self.workspace is None or self.workspace.numel() * self.workspace.element_size() < nb:
            with torch.cuda.device(self.device):
                self.workspace = torch.zeros((nb + 3) // 4, dtype=torch.float32, device=self.device)
        _fused.launch("rover_lidar_prepare", self.device, self._h, self.workspace.data_ptr(), nb)
        return self

    def cast(self, range_out: torch.Tensor, hits_out: torch.Tensor | None = None) -> torch.Tensor:
        n, R = self.num_envs, self.rays
        if self.workspace is None:
            raise RuntimeError("Lidar.cast needs prepare() (or an adopted workspace) first")
        pitch = _fused.row_pitch("range_out", range_out, R, rows=n, device=self.table.device)
        if hits_out is not None:
            _fused.f32_cuda("hits_out", hits_out, self.table.device, "the lidar's device")
            _fused.holds("hits_out", hits_out, (n, R, 3))
        _fused.launch("rover_lidar_cast", self.device, self._h, C.byref(self.native), self.workspace.data_ptr(),
                      self.table.data_ptr(), range_out.data_ptr(), pitch, _fused.ptr(hits_out))
        return range_out
