"""A rolling, robot-centric elevation map built from the on-board depth camera, as ONE HIP launch per env step (C ABI:
``include/rover_elevation.h``).

The policy reads a 31 x 31 height scan around the rover.  The simulator's scan is an oracle: vertical rays with perfect knowledge
all round.  A real rover has the depth camera; it builds an elevation map from depth and odometry and feeds the policy from that
map.  ``ElevationMap.update`` is that link: scroll the world-anchored, toroidally addressed map to the new pose, unproject the
depth image with a caller-supplied table of Body-frame rays, reduce the points to one height (the maximum) per cell, fuse it into
the map and read the scan out of the result.  ``RoverEnv`` runs it behind the camera's render -> sensor -> noise / clip chain when
``cfg.elevation`` is set and publishes ``extras["elevation_scan"]`` / ``["elevation_known"]`` / ``["elevation_count"]``;
``policy_rows`` puts such a scan into observation rows, so a trained actor can be evaluated on what the camera can see.
``ElevationMap.fill`` is the inpainting pass behind it (``include/rover_elevation_fill.h``): one more launch that fills the unknown
cells of the window with the minimum of their known neighbours, ring by ring, and reports how far each value was carried.
``ElevationMap.traverse`` (``include/rover_elevation_traverse.h``) derives from the map, or from the fill's window, where the rover
may drive: slope, step height, roughness and a cost per cell, and the scan of the cost, again as one launch.

``TorchElevationMap`` is the same interface in plain numpy on float32, every operation in the header's order: the specification
of the kernel, compared bit for bit, and it runs on the CPU.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _fused, _lib

_QNAN = np.uint32(0x7FC00000)
_CELL_CAP = 1073741824.0           # cells are clamped to +-2^30 (include/rover_elevation.h)


def _quat_to_mat64(q) -> np.ndarray:
    w, x, y, z = (np.asarray(q, dtype=np.float64) / np.linalg.norm(np.asarray(q, dtype=np.float64)))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def body_rays(camera_cfg, dtype=np.float32) -> np.ndarray:
    """The (height * width, 3) table of unit ray directions in the Body frame, pixel (row i, column j) at i * width + j: the
    pinhole through each pixel centre in the USD camera frame (x right, y up, looking along -z; row 0 at the top), turned by the
    mount orientation.  Computed in float64 and rounded once; the device and the specification consume this same array."""
    fx, fy = camera_cfg.focal_px
    W, H = int(camera_cfg.width), int(camera_cfg.height)
    u = (np.arange(W, dtype=np.float64) + 0.5 - 0.5 * W) / fx
    v = -(np.arange(H, dtype=np.float64) + 0.5 - 0.5 * H) / fy
    U, V = np.meshgrid(u, v, indexing="xy")
    d = np.stack([U, V, -np.ones_like(U)], -1)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return np.ascontiguousarray((d @ _quat_to_mat64(camera_cfg.orientation).T).reshape(H * W, 3), dtype=dtype)


def scan_offsets(scanner_cfg, dtype=np.float32):
    """(ray_x (nx,), ray_y (ny,)): the height scanner's grid offsets as the oracle forms them, in double from the fp32 size and
    resolution, rounded once."""
    nx, ny = scanner_cfg.grid
    res = float(np.float32(scanner_cfg.resolution))
    sx, sy = float(np.float32(scanner_cfg.size[0])), float(np.float32(scanner_cfg.size[1]))
    return ((-0.5 * sx + res * np.arange(nx, dtype=np.float64)).astype(dtype),
            (-0.5 * sy + res * np.arange(ny, dtype=np.float64)).astype(dtype))


def policy_rows(obs: torch.Tensor, scan: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Observation rows ``(n, 4 + rays)`` with the height-scan columns replaced by ``scan`` ``(n, rays)``; the four columns in
    front (actions, distance, heading) are copied."""
    if obs.dim() != 2 or scan.dim() != 2 or obs.shape[0] != scan.shape[0] or obs.shape[1] != 4 + scan.shape[1]:
        raise ValueError("obs must be (n, 4 + rays) and scan (n, rays)")
    if out is None:
        out = torch.empty_like(obs)
    elif out.shape != obs.shape:
        raise ValueError("out must have obs's shape")
    out[:, :4] = obs[:, :4]
    out[:, 4:] = scan
    return out


class _ElevationBase:
    def __init__(self, cfg, camera_cfg, scanner_cfg, num_envs: int, rays=None):
        self.map_cfg, self.camera_cfg, self.scanner_cfg = cfg, camera_cfg, scanner_cfg
        self.cfg = cfg.to_native(camera_cfg.position, scanner_cfg.height_offset)
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError("num_envs must be >= 1")
        self.height, self.width = int(camera_cfg.height), int(camera_cfg.width)
        if self.height < 1 or self.width < 1 or self.pixels > _lib.ELEVATION_MAX_PIXELS:
            raise ValueError(f"height * width must be in [1, {_lib.ELEVATION_MAX_PIXELS}]")
        self.nx, self.ny = (int(v) for v in scanner_cfg.grid)
        if self.nx * self.ny > _lib.ELEVATION_MAX_RAYS:
            raise ValueError(f"the scan must have at most {_lib.ELEVATION_MAX_RAYS} rays")
        self.grid = int(self.cfg.grid)
        self._rays32 = body_rays(camera_cfg) if rays is None else np.ascontiguousarray(rays, dtype=np.float32)
        if self._rays32.shape != (self.pixels, 3):
            raise ValueError(f"rays must be ({self.pixels}, 3)")
        self._ray_x32, self._ray_y32 = scan_offsets(scanner_cfg)

    @property
    def pixels(self) -> int:
        return self.height * self.width

    @property
    def columns(self) -> int:
        return self.nx * self.ny


class TorchElevationMap(_ElevationBase):
    """The CPU specification of ``ElevationMap``: numpy float32, one rounding per operation in the header's order.  ``map`` is
    ``(n, grid, grid)`` (NaN = unknown), ``origin`` ``(n, 2)`` int32.  ``update`` and ``scan`` take numpy arrays (or CPU tensors):
    depth ``(n, height * width)`` or ``(n, height, width)``, pos ``(n, 3)``, quat ``(n, 4)``, and return ``(scan, known, count)``.
    With ``float64=True`` everything runs in float64 on the unrounded parameters and a float64 ray table: the reference of the one
    tolerance test."""

    def __init__(self, cfg, camera_cfg, scanner_cfg, num_envs: int, device=None, float64: bool = False, rays=None):
        super().__init__(cfg, camera_cfg, scanner_cfg, num_envs, rays)
        self.float64 = bool(float64)
        ft = self.ft = np.float64 if self.float64 else np.float32
        c = self.cfg
        if self.float64:
            self.rays = body_rays(camera_cfg, np.float64) if rays is None else np.asarray(rays, dtype=np.float64)
            self.ray_x, self.ray_y = scan_offsets(scanner_cfg, np.float64)
            self.inv_cell, self.mount = 1.0 / float(cfg.cell), np.array(camera_cfg.position, dtype=np.float64)
            self.alpha, self.height_offset = float(cfg.alpha), float(scanner_cfg.height_offset)
        else:
            self.rays, self.ray_x, self.ray_y = self._rays32, self._ray_x32, self._ray_y32
            self.inv_cell, self.mount = ft(c.inv_cell), np.array(list(c.mount_pos), dtype=ft)
            self.alpha, self.height_offset = ft(c.alpha), ft(c.height_offset)
        self.range_min, self.range_max, self.unknown_value = ft(c.range_min), ft(c.range_max), ft(c.unknown_value)
        self.map = np.full((self.num_envs, self.grid, self.grid), np.nan, dtype=ft)
        self.origin = np.zeros((self.num_envs, 2), dtype=np.int32)

    # ---------------------------------------------------------------------------------------------------------- pieces
    def _nan(self):
        return np.nan if self.float64 else _QNAN.view(np.float32)

    def cells(self, v: np.ndarray) -> np.ndarray:
        """The global cell of each (finite) coordinate, int64; a non-finite one gives 0."""
        with np.errstate(all="ignore"):
            f = np.floor(v * self.inv_cell)
            f = np.where(np.isfinite(v), np.minimum(np.maximum(f, self.ft(-_CELL_CAP)), self.ft(_CELL_CAP)), 0)
        return f.astype(np.int64)

    @staticmethod
    def keys(v: np.ndarray) -> np.ndarray:
        b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
        return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))

    @staticmethod
    def values(k: np.ndarray) -> np.ndarray:
        return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)

    def _pose(self, pos, quat):
        as_np = lambda t: t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)      # noqa: E731
        pos, quat = as_np(pos).astype(self.ft).reshape(self.num_envs, 3), as_np(quat).astype(self.ft).reshape(self.num_envs, 4)
        return pos, quat, np.isfinite(pos).all(1) & np.isfinite(quat).all(1)

    def points(self, depth, pos, quat):
        """(valid (n, hw), world points wx, wy, wz (n, hw)) of step 4, before the window test."""
        ft, n = self.ft, self.num_envs
        d = (depth.numpy() if isinstance(depth, torch.Tensor) else np.asarray(depth)).reshape(n, self.pixels).astype(ft)
        with np.errstate(all="ignore"):
            valid = np.isfinite(d) & (d >= self.range_min) & (d <= self.range_max)
            r, m = self.rays, self.mount
            bx, by, bz = m[0] + d * r[:, 0], m[1] + d * r[:, 1], m[2] + d * r[:, 2]
            w, x, y, z = (quat[:, i, None] for i in range(4))
            one, two = ft(1.0), ft(2.0)
            r00, r01, r02 = one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)
            r10, r11, r12 = two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)
            r20, r21, r22 = two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)
            wx = pos[:, 0, None] + ((r00 * bx + r01 * by) + r02 * bz)
            wy = pos[:, 1, None] + ((r10 * bx + r11 * by) + r12 * bz)
            wz = pos[:, 2, None] + ((r20 * bx + r21 * by) + r22 * bz)
            valid &= np.isfinite(wx) & np.isfinite(wy) & np.isfinite(wz)
        return valid, wx, wy, wz

    def _columns(self, origin, pos, quat, ok):
        """Step 8's look-up: (inside (n, ny, nx) bool, the index triple of each column's slot)."""
        ft, n, G = self.ft, self.num_envs, self.grid
        with np.errstate(all="ignore"):
            w, x, y, z = (quat[:, i] for i in range(4))
            one, two = ft(1.0), ft(2.0)
            a = one - two * (y * y + z * z)
            b = two * (w * z + x * y)
            inv = one / np.sqrt(a * a + b * b)
            cy, sy = (a * inv)[:, None, None], (b * inv)[:, None, None]
            ox, oy = self.ray_x[None, None, :], self.ray_y[None, :, None]
            sx_ = pos[:, 0, None, None] + (cy * ox - sy * oy)
            sy_ = pos[:, 1, None, None] + (sy * ox + cy * oy)
            fin = np.isfinite(sx_) & np.isfinite(sy_) & ok[:, None, None]
        gx, gy = self.cells(sx_), self.cells(sy_)
        lo = origin.astype(np.int64) - G // 2
        dx, dy = gx - lo[:, 0, None, None], gy - lo[:, 1, None, None]
        inside = fin & (dx >= 0) & (dx < G) & (dy >= 0) & (dy < G)
        return inside, (np.arange(n)[:, None, None], gy & (G - 1), gx & (G - 1))

    def _read(self, mp, origin, pos, quat, ok, dist=None):
        """Step 8 on ``mp`` / ``origin``: (scan (n, ny * nx), known uint8, count int32).  With ``dist`` (the fill's bytes per slot) a
        cell is known where its dist is below 255, and the middle result is the columns' dist, 255 where unknown."""
        ft, n = self.ft, self.num_envs
        inside, at = self._columns(origin, pos, quat, ok)
        h = mp[at]
        known = inside & (~np.isnan(h) if dist is None else dist[at] < 255)
        with np.errstate(all="ignore"):
            out = np.where(known, (pos[:, 2, None, None] - h) - self.height_offset, self.unknown_value).astype(ft)
        mid = known.astype(np.uint8) if dist is None else np.where(known, dist[at], 255).astype(np.uint8)
        known = known.reshape(n, -1)
        return out.reshape(n, -1), mid.reshape(n, -1), known.sum(1).astype(np.int32)

    # --------------------------------------------------------------------------------------------------------- methods
    def update(self, depth, pos, quat, reset=(None, None), scan_out=None, known_out=None, count_out=None):
        ft, n, G = self.ft, self.num_envs, self.grid
        pos, quat, ok = self._pose(pos, quat)
        flag = np.zeros(n, dtype=bool)
        for r in (reset or ()):
            if r is not None:
                flag |= (r.numpy() if isinstance(r, torch.Tensor) else np.asarray(r)).reshape(n).astype(bool)
        nan = self._nan()
        self.map[flag & ~ok] = nan                                           # step 2
        c = np.stack([self.cells(pos[:, 0]), self.cells(pos[:, 1])], 1)     # step 3
        s = np.arange(G, dtype=np.int64)
        lo_new, lo_old = c - G // 2, self.origin.astype(np.int64) - G // 2
        denotes = lambda lo: lo[:, None] + ((s[None, :] - lo[:, None]) & (G - 1))      # noqa: E731
        same_x, same_y = denotes(lo_new[:, 0]) == denotes(lo_old[:, 0]), denotes(lo_new[:, 1]) == denotes(lo_old[:, 1])
        keep = same_y[:, :, None] & same_x[:, None, :] & ~flag[:, None, None]
        v = np.where(keep, self.map, nan).astype(ft)
        if depth is not None:                                                # steps 4 - 6
            valid, wx, wy, wz = self.points(depth, pos, quat)
            gx, gy = self.cells(wx), self.cells(wy)
            dx, dy = gx - lo_new[:, 0, None], gy - lo_new[:, 1, None]
            valid &= (dx >= 0) & (dx < G) & (dy >= 0) & (dy < G) & ok[:, None]
            e = np.broadcast_to(np.arange(n)[:, None], valid.shape)[valid]
            slot = (e * G + (gy[valid] & (G - 1))) * G + (gx[valid] & (G - 1))
            touched = np.zeros(n * G * G, dtype=bool)
            touched[slot] = True
            if self.float64:
                frame = np.full(n * G * G, -np.inf)
                np.maximum.at(frame, slot, wz[valid])
            else:
                k = np.zeros(n * G * G, dtype=np.uint32)
                np.maximum.at(k, slot, self.keys(wz[valid]))
                frame = self.values(k)
            touched, frame = touched.reshape(n, G, G), frame.reshape(n, G, G)
            with np.errstate(all="ignore"):
                blend = v + self.alpha * (frame - v)
            fused = np.where(np.isnan(v) | (self.alpha == 1.0), frame, blend)
            v = np.where(touched, fused, v).astype(ft)
        v = np.where(np.isnan(v), nan, v).astype(ft)
        self.map[ok] = v[ok]                                                 # step 7
        self.origin[ok] = c[ok].astype(np.int32)
        return self._emit(self._read(self.map, self.origin, pos, quat, ok), scan_out, known_out, count_out)

    def scan(self, pos, quat, scan_out=None, known_out=None, count_out=None):
        pos, quat, ok = self._pose(pos, quat)
        return self._emit(self._read(self.map, self.origin, pos, quat, ok), scan_out, known_out, count_out)

    def fill_window(self, iterations: int):
        """Steps 1 - 3 of include/rover_elevation_fill.h on ``map`` / ``origin``, which stay as they are: (filled (n, G, G) float32,
        dist (n, G, G) uint8), both in the map's slot order."""
        if self.float64:
            raise ValueError("the fill is specified on float32 (its minimum is one of key bits)")
        if not 1 <= int(iterations) <= _lib.ELEVATION_FILL_MAX_ITERATIONS:
            raise ValueError(f"iterations must be in [1, {_lib.ELEVATION_FILL_MAX_ITERATIONS}]")
        n, G = self.num_envs, self.grid
        lo = self.origin.astype(np.int64) - G // 2
        w = np.arange(G, dtype=np.int64)
        at = (np.arange(n)[:, None, None], ((lo[:, 1, None] + w) & (G - 1))[:, :, None], ((lo[:, 0, None] + w) & (G - 1))[:, None, :])
        h = self.map[at]                                                     # window order: [e, i over y, j over x]
        dist = np.where(np.isnan(h), 255, 0).astype(np.int64)
        none = np.uint32(0xFFFFFFFF)                                         # above the key of every float that is not a NaN
        for k in range(1, int(iterations) + 1):
            framed = np.full((n, G + 2, G + 2), none, dtype=np.uint32)       # the frame: outside the window nothing counts
            framed[:, 1:-1, 1:-1] = np.where(dist < k, self.keys(h), none)
            best = np.minimum.reduce([framed[:, 1 + di:1 + di + G, 1 + dj:1 + dj + G]
                                      for di in (-1, 0, 1) for dj in (-1, 0, 1) if di or dj])
            take = (dist == 255) & (best != none)
            if not take.any():
                break
            h = np.where(take, self.values(best), h)
            dist = np.where(take, k, dist)
        filled, cell_dist = np.empty_like(self.map), np.empty(self.map.shape, dtype=np.uint8)
        filled[at], cell_dist[at] = h, dist
        return filled, cell_dist

    def fill(self, pos, quat, scan_out=None, dist_out=None, count_out=None, filled_out=None, cell_dist_out=None, iterations=None):
        """The min-fill of the map's window and the scan of the filled window (include/rover_elevation_fill.h); ``iterations``
        defaults to the cfg's ``fill_iterations``.  Returns (scan, dist (n, rays) uint8, count, filled (n, G, G), cell_dist
        (n, G, G) uint8)."""
        filled, cell_dist = self.fill_window(self.map_cfg.fill_iterations if iterations is None else iterations)
        pos, quat, ok = self._pose(pos, quat)
        res = (*self._read(filled, self.origin, pos, quat, ok, dist=cell_dist), filled, cell_dist)
        return self._emit(res, scan_out, dist_out, count_out, filled_out, cell_dist_out)

    def _traverse_cfg(self, cfg):
        cfg = self.map_cfg.traverse if cfg is None else cfg
        if cfg is None:
            raise ValueError("traverse needs a TraverseCfg (ElevationMapCfg.traverse or cfg=)")
        return cfg.to_native()

    def _heights(self, heights):
        if heights is None:
            return self.map
        h = heights.numpy() if isinstance(heights, torch.Tensor) else np.asarray(heights)
        if h.dtype != np.float32 or h.size != self.map.size:
            raise ValueError(f"heights must be float32 of {self.map.size} values")
        return h.reshape(self.map.shape)

    def traverse_window(self, heights=None, cfg=None):
        """Steps 1 - 4 of include/rover_elevation_traverse.h on ``heights`` ((n, G, G) float32 in slot order; ``None``: the map) and
        ``origin``: (slope, step, rough, cost (n, G, G) float32, class (n, G, G) uint8), all in slot order."""
        if self.float64:
            raise ValueError("the traverse layers are specified on float32")
        t, ft, n, G = self._traverse_cfg(cfg), np.float32, self.num_envs, self.grid
        r, cell, inv_cell = int(t.radius), ft(self.cfg.cell), ft(self.cfg.inv_cell)
        lo = self.origin.astype(np.int64) - G // 2
        w = np.arange(G, dtype=np.int64)
        at = (np.arange(n)[:, None, None], ((lo[:, 1, None] + w) & (G - 1))[:, :, None], ((lo[:, 0, None] + w) & (G - 1))[:, None, :])
        h = self._heights(heights)[at]                                       # window order: [e, i over y, j over x]
        nan = _QNAN.view(np.float32)
        framed = np.full((n, G + 2 * r, G + 2 * r), nan, dtype=ft)           # the frame: outside the window nothing is usable
        framed[:, r:r + G, r:r + G] = h
        shifted = lambda di, dj: framed[:, r + di:r + di + G, r + dj:r + dj + G]      # noqa: E731
        with np.errstate(all="ignore"):
            def one_sided(lower, upper):
                l, u = np.isfinite(lower), np.isfinite(upper)
                both, up, down = (upper - lower) * (ft(0.5) * inv_cell), (upper - h) * inv_cell, (h - lower) * inv_cell
                return np.where(l & u, both, np.where(u, up, np.where(l, down, ft(0.0)))).astype(ft)

            gx, gy = one_sided(shifted(0, -1), shifted(0, 1)), one_sided(shifted(-1, 0), shifted(1, 0))
            slope = np.sqrt((gx * gx) + (gy * gy))
            kmin, kmax = np.full(h.shape, 0xFFFFFFFF, dtype=np.uint32), np.zeros(h.shape, dtype=np.uint32)
            support, acc = np.zeros(h.shape, dtype=np.int64), np.zeros(h.shape, dtype=ft)
            for di in range(-r, r + 1):
                for dj in range(-r, r + 1):
                    hd = shifted(di, dj)
                    ok = np.isfinite(hd)
                    k = self.keys(hd)
                    kmin, kmax = np.where(ok, np.minimum(kmin, k), kmin), np.where(ok, np.maximum(kmax, k), kmax)
                    support += ok
                    if di or dj:
                        res = (hd - h) - ((gx * (ft(dj) * cell)) + (gy * (ft(di) * cell)))
                        acc = np.where(ok, acc + res * res, acc).astype(ft)
            step = self.values(kmax) - self.values(kmin)
            cnt = support - 1
            rough = np.where(cnt == 0, ft(0.0), np.sqrt(acc / cnt.astype(ft))).astype(ft)
            sc, tc, rc = ft(t.slope_crit), ft(t.step_crit), ft(t.rough_crit)
            lethal = ~((slope < sc) & (step < tc) & (rough < rc))
            total = ((ft(t.w_slope) * (slope / sc)) + (ft(t.w_step) * (step / tc))) + (ft(t.w_rough) * (rough / rc))
            cost = np.where(lethal, ft(1.0), np.fmin(total, ft(1.0))).astype(ft)
        verdict = np.isfinite(h) & (support >= int(t.min_support))
        cls = np.where(verdict, np.where(lethal, 2, 1), 0).astype(np.uint8)
        out = []
        for layer in (slope, step, rough, cost):
            slots = np.empty((n, G, G), dtype=ft)
            slots[at] = np.where(verdict, layer, nan)
            out.append(slots)
        cls_slots = np.empty((n, G, G), dtype=np.uint8)
        cls_slots[at] = cls
        return (*out, cls_slots)

    def traverse(self, pos, quat, heights=None, scan_out=None, class_out=None, count_out=None, slope_out=None, step_out=None,
                 rough_out=None, cost_out=None, cfg=None):
        """The layers of ``heights`` (``None``: the map) and the scan of the cost (include/rover_elevation_traverse.h); ``cfg``
        defaults to the map cfg's ``traverse``.  Returns (cost scan (n, rays), class (n, rays) uint8, lethal count (n,) int32, slope,
        step, rough, cost (n, G, G))."""
        t = self._traverse_cfg(cfg)
        slope, step, rough, cost, cls = self.traverse_window(heights, cfg)
        pos, quat, ok = self._pose(pos, quat)
        inside, at = self._columns(self.origin, pos, quat, ok)
        col_cls = np.where(inside, cls[at], 0).astype(np.uint8)
        scan = np.where(col_cls > 0, cost[at], np.float32(t.unknown_cost)).astype(np.float32)
        n = self.num_envs
        res = (scan.reshape(n, -1), col_cls.reshape(n, -1), (col_cls == 2).reshape(n, -1).sum(1).astype(np.int32), slope, step, rough, cost)
        return self._emit(res, scan_out, class_out, count_out, slope_out, step_out, rough_out, cost_out)

    @staticmethod
    def _emit(res, *outs):
        for src, dst in zip(res, outs):
            if dst is not None:
                (dst.numpy() if isinstance(dst, torch.Tensor) else dst)[...] = src.reshape(dst.shape)
        return res

    def clear(self, mask=None):
        if mask is None:
            self.map[...] = self._nan()
        else:
            self.map[(mask.numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)).astype(bool)] = self._nan()

    def state_dict(self) -> dict:
        return {"elevation_map": torch.from_numpy(self.map.copy()), "elevation_origin": torch.from_numpy(self.origin.copy())}

    def load_state_dict(self, sd: dict):
        self.map[...] = sd["elevation_map"].cpu().numpy().reshape(self.map.shape)
        self.origin[...] = sd["elevation_origin"].cpu().numpy().reshape(self.origin.shape)


class ElevationMap(_ElevationBase):
    """The device class.  ``update`` is one asynchronous ``rover_elevation_step`` launch on the current stream, ``scan`` one
    ``rover_elevation_scan`` launch.

    ``depth``: ``None`` (no frame: scroll and scan only) or a float32 cuda tensor, contiguous ``(n, height, width)`` or
    ``(n, height * width)`` with unit column stride and any row pitch.  ``pos`` ``(n, 3)`` and ``quat`` ``(n, 4)``: float32 cuda
    views with the SAME two strides -- ``state[POS:POS + 3].t()`` / ``state[QUAT:QUAT + 4].t()`` of the env's SoA state, or
    ``poses[:, :3]`` / ``poses[:, 3:]`` of an ``(n, 7)`` array.  ``reset``: up to two uint8 / bool cuda tensors of ``n`` flags,
    OR-ed.  ``scan_out`` ``(n, rays)`` float32 with unit column stride and any row pitch (columns 4 ... of an observation row, for
    one), ``known_out`` contiguous ``(n, rays)`` uint8, ``count_out`` contiguous ``(n,)`` int32; each is allocated where
    the caller gives none.  Returns ``(scan, known, count)``."""

    def __init__(self, cfg, camera_cfg, scanner_cfg, num_envs: int, device="cuda", rays=None):
        super().__init__(cfg, camera_cfg, scanner_cfg, num_envs, rays)
        _fused.require_gpu("ElevationMap", "TorchElevationMap is the CPU specification")
        self._lib = _lib.load()
        self.device = torch.device(device)
        n, G = self.num_envs, self.grid
        with torch.cuda.device(self.device):
            self.map = torch.full((n, G, G), float("nan"), dtype=torch.float32, device=self.device)
            self.origin = torch.zeros((n, 2), dtype=torch.int32, device=self.device)
            self.rays = torch.from_numpy(self._rays32).to(self.device)
            self.ray_x = torch.from_numpy(self._ray_x32).to(self.device)
            self.ray_y = torch.from_numpy(self._ray_y32).to(self.device)

    def _f32(self, t, name: str, cols: int):
        """(pointer, row pitch) of a float32 cuda ``(n, cols)`` tensor with unit column stride."""
        pitch = _fused.row_pitch(name, t, cols, rows=self.num_envs, device=self.map.device)
        return t.data_ptr(), pitch

    def _pose(self, pos, quat):
        n = self.num_envs
        for t, k, nm in ((pos, 3, "pos"), (quat, 4, "quat")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.device != self.map.device or \
                    tuple(t.shape) != (n, k):
                raise ValueError(f"{nm} must be a float32 cuda ({n}, {k}) tensor on the map's device")
        cs, es = pos.stride(1), (pos.stride(0) if n > 1 else 1)             # one env: the env stride is not read
        if (n > 1 and quat.stride(0) != es) or quat.stride(1) != cs or cs < 1 or es < 1:
            raise ValueError("pos and quat must share their two strides, both positive")
        return pos.data_ptr(), quat.data_ptr(), int(cs), int(es)

    def _outs(self, scan_out, known_out, count_out):
        """((scan, known, count), scan pointer, scan pitch), each buffer allocated where the caller gave none."""
        n, cols, dev = self.num_envs, self.columns, self.map.device
        if scan_out is None:
            scan_out = torch.empty((n, cols), dtype=torch.float32, device=dev)
        if known_out is None:
            known_out = torch.empty((n, cols), dtype=torch.uint8, device=dev)
        if count_out is None:
            count_out = torch.empty(n, dtype=torch.int32, device=dev)
        for t, dt, num, nm in ((known_out, torch.uint8, n * cols, "known_out"), (count_out, torch.int32, n, "count_out")):
            if not t.is_cuda or t.device != dev or t.dtype != dt or not t.is_contiguous() or t.numel() != num:
                raise ValueError(f"{nm} must be a contiguous {dt} cuda tensor of {num} values on the map's device")
        ptr, pitch = self._f32(scan_out, "scan_out", cols)
        return (scan_out, known_out, count_out), ptr, pitch

    def _flags(self, r):
        if r is None:
            return None
        if not isinstance(r, torch.Tensor) or not r.is_cuda or r.device != self.map.device or not r.is_contiguous() or \
                r.dtype not in (torch.uint8, torch.bool) or r.numel() != self.num_envs:
            raise ValueError(f"a reset flag tensor must be a contiguous uint8 / bool cuda tensor of {self.num_envs} flags")
        return r.data_ptr()

    def update(self, depth, pos, quat, reset=(None, None), scan_out=None, known_out=None, count_out=None):
        reset = tuple(reset or ()) + (None, None)
        if len(reset) > 4 or any(r is not None for r in reset[2:]):
            raise ValueError("reset takes at most two flag tensors")
        d_ptr, pitch = (None, self.pixels) if depth is None else self._f32(depth, "depth", self.pixels)
        p_ptr, q_ptr, cs, es = self._pose(pos, quat)
        outs, s_ptr, s_pitch = self._outs(scan_out, known_out, count_out)
        _fused.launch("rover_elevation_step", self.map.device, self.cfg, d_ptr, int(pitch), self.height, self.width,
                      self.rays.data_ptr(), p_ptr, q_ptr, cs, es, self._flags(reset[0]), self._flags(reset[1]), self.map.data_ptr(),
                      self.origin.data_ptr(), self.ray_x.data_ptr(), self.nx, self.ray_y.data_ptr(), self.ny, s_ptr, int(s_pitch),
                      _fused.ptr(outs[1]), _fused.ptr(outs[2]), self.num_envs)
        return outs

    def scan(self, pos, quat, scan_out=None, known_out=None, count_out=None):
        p_ptr, q_ptr, cs, es = self._pose(pos, quat)
        outs, s_ptr, s_pitch = self._outs(scan_out, known_out, count_out)
        _fused.launch("rover_elevation_scan", self.map.device, self.cfg, p_ptr, q_ptr, cs, es, self.map.data_ptr(),
                      self.origin.data_ptr(), self.ray_x.data_ptr(), self.nx, self.ray_y.data_ptr(), self.ny, s_ptr, int(s_pitch),
                      _fused.ptr(outs[1]), _fused.ptr(outs[2]), self.num_envs)
        return outs

    def fill(self, pos, quat, scan_out=None, dist_out=None, count_out=None, filled_out=None, cell_dist_out=None, iterations=None):
        """One asynchronous ``rover_elevation_fill`` launch: the min-fill of the map's window, at most ``iterations`` cells far
        (default: the cfg's ``fill_iterations``), and the scan of the filled window.  ``map`` and ``origin`` are only read.
        ``scan_out`` / ``dist_out`` (uint8, 0 measured, k filled in sweep k, 255 unknown) / ``count_out`` as ``update``'s three,
        allocated where the caller gives none.  ``filled_out`` (n, G, G) float32 and ``cell_dist_out`` (n, G, G) uint8, both
        contiguous and in the map's slot order, are written only where given (``True``: allocated here).  Returns (scan, dist,
        count, filled, cell_dist), the last two ``None`` where not asked for."""
        n, G, dev = self.num_envs, self.grid, self.map.device
        fc = _lib.ElevationFillCfg(int(self.map_cfg.fill_iterations if iterations is None else iterations))
        if not 1 <= fc.iterations <= _lib.ELEVATION_FILL_MAX_ITERATIONS:
            raise ValueError(f"iterations must be in [1, {_lib.ELEVATION_FILL_MAX_ITERATIONS}]")
        p_ptr, q_ptr, cs, es = self._pose(pos, quat)
        outs, s_ptr, s_pitch = self._outs(scan_out, dist_out, count_out)
        if filled_out is True:
            filled_out = torch.empty((n, G, G), dtype=torch.float32, device=dev)
        if cell_dist_out is True:
            cell_dist_out = torch.empty((n, G, G), dtype=torch.uint8, device=dev)
        for t, dt, nm in ((filled_out, torch.float32, "filled_out"), (cell_dist_out, torch.uint8, "cell_dist_out")):
            if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev or t.dtype != dt or
                                  not t.is_contiguous() or t.numel() != n * G * G):
                raise ValueError(f"{nm} must be a contiguous {dt} cuda tensor of {n * G * G} values on the map's device")
        _fused.launch("rover_elevation_fill", dev, self.cfg, fc, p_ptr, q_ptr, cs, es, self.map.data_ptr(), self.origin.data_ptr(),
                      self.ray_x.data_ptr(), self.nx, self.ray_y.data_ptr(), self.ny, s_ptr, int(s_pitch), _fused.ptr(outs[1]),
                      _fused.ptr(outs[2]), _fused.ptr(filled_out), _fused.ptr(cell_dist_out), n)
        return (*outs, filled_out, cell_dist_out)

    def traverse(self, pos, quat, heights=None, scan_out=None, class_out=None, count_out=None, slope_out=None, step_out=None,
                 rough_out=None, cost_out=None, cfg=None):
        """One asynchronous ``rover_elevation_traverse`` launch: slope, step height, roughness and cost of ``heights`` (a contiguous
        float32 (n, G, G) cuda tensor in the map's slot order, such as ``fill``'s ``filled_out``; ``None``: the map) under ``cfg``
        (default: the map cfg's ``traverse``), and the scan of the cost.  ``heights``, ``map`` and ``origin`` are only read.
        ``scan_out`` (the cost under each scan column, ``unknown_cost`` where there is none) / ``class_out`` (uint8: 0 no verdict,
        1 free, 2 lethal) / ``count_out`` (the lethal columns) as ``update``'s three, allocated where the caller gives none;
        ``scan_out=False``: no scan, the three are ``None``.  The four window outputs, contiguous (n, G, G) float32 in slot order,
        NaN where a cell has no verdict, are written only where given (``True``: allocated here).  Returns (scan, class, count,
        slope, step, rough, cost)."""
        n, G, dev = self.num_envs, self.grid, self.map.device
        if cfg is None:
            cfg = self.map_cfg.traverse
        if cfg is None:
            raise ValueError("traverse needs a TraverseCfg (ElevationMapCfg.traverse or cfg=)")
        tc = cfg.to_native()
        if heights is None:
            heights = self.map
        elif not isinstance(heights, torch.Tensor) or not heights.is_cuda or heights.device != dev or heights.dtype != torch.float32 or \
                not heights.is_contiguous() or heights.numel() != n * G * G:
            raise ValueError(f"heights must be a contiguous float32 cuda tensor of {n * G * G} values on the map's device")
        p_ptr, q_ptr, cs, es = self._pose(pos, quat)
        if scan_out is False:
            if class_out is not None or count_out is not None:
                raise ValueError("class_out and count_out are written only with a scan")
            outs, s_ptr, s_pitch = (None, None, None), None, self.columns
        else:
            outs, s_ptr, s_pitch = self._outs(scan_out, class_out, count_out)
        layers = []
        for t, nm in ((slope_out, "slope_out"), (step_out, "step_out"), (rough_out, "rough_out"), (cost_out, "cost_out")):
            if t is True:
                t = torch.empty((n, G, G), dtype=torch.float32, device=dev)
            if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev or t.dtype != torch.float32 or
                                  not t.is_contiguous() or t.numel() != n * G * G):
                raise ValueError(f"{nm} must be a contiguous float32 cuda tensor of {n * G * G} values on the map's device")
            layers.append(t)
        if s_ptr is None and all(t is None for t in layers):
            raise ValueError("traverse needs the scan or one of the four window outputs")
        _fused.launch("rover_elevation_traverse", dev, self.cfg, tc, p_ptr, q_ptr, cs, es, heights.data_ptr(), self.origin.data_ptr(),
                      self.ray_x.data_ptr(), self.nx, self.ray_y.data_ptr(), self.ny, s_ptr, int(s_pitch), _fused.ptr(outs[1]),
                      _fused.ptr(outs[2]), *(_fused.ptr(t) for t in layers), n)
        return (*outs, *layers)

    def clear(self, mask=None):
        """All maps (or those of ``mask``) back to unknown."""
        if mask is None:
            self.map.fill_(float("nan"))
        else:
            self.map[mask.to(device=self.map.device, dtype=torch.bool)] = float("nan")

    def state_dict(self) -> dict:
        return {"elevation_map": self.map.detach().cpu().clone(), "elevation_origin": self.origin.detach().cpu().clone()}

    def load_state_dict(self, sd: dict):
        if sd["elevation_map"].shape != self.map.shape or sd["elevation_origin"].shape != self.origin.shape:
            raise ValueError("the checkpoint's elevation map was taken from another size of env or grid")
        self.map.copy_(sd["elevation_map"].to(self.map.device))
        self.origin.copy_(sd["elevation_origin"].to(self.origin.device))
