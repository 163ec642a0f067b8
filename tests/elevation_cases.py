"""Shared inputs of the elevation-map tests (tests/test_elevation.py, tests/test_gpu_elevation.py, tests/test_gpu_elevation_env.py):
configurations, poses, depth images of a plane, and the corridor of scan columns the camera must fill in one frame."""
from __future__ import annotations

import numpy as np

from isaac_rover_orbit_amd import elevation
from isaac_rover_orbit_amd.cfg import CameraCfg, ElevationMapCfg, RayCasterCfg


def cfgs(H=90, W=160, G=64, **kw):
    """(ElevationMapCfg, CameraCfg, RayCasterCfg): the default camera's lens and mount at another image size."""
    return ElevationMapCfg(grid=G, **kw), CameraCfg(width=W, height=H), RayCasterCfg()


def quat(yaw, pitch=0.0, roll=0.0) -> np.ndarray:
    """(w, x, y, z) float32 of the z-y-x Euler angles."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    return np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                     cr * cp * sy - sr * sp * cy], dtype=np.float32)


def plane_depth(cam, pos, quats, ground=0.0, rays=None) -> np.ndarray:
    """(n, H * W) float32 range images of the horizontal plane z = ground, +inf above the horizon; float64 inside."""
    r = elevation.body_rays(cam, np.float64) if rays is None else np.asarray(rays, np.float64)
    out = []
    for p, q in zip(np.asarray(pos, np.float64), np.asarray(quats, np.float64)):
        R = elevation._quat_to_mat64(q)
        o, d = p + R @ np.asarray(cam.position, np.float64), r @ R.T
        with np.errstate(divide="ignore"):
            t = (ground - o[2]) / d[:, 2]
        out.append(np.where((d[:, 2] < 0) & (t > 0), t, np.inf))
    return np.stack(out).astype(np.float32)


def random_depth(rng, n, hw, lo=0.3, hi=4.0, holes=0.1) -> np.ndarray:
    d = (lo + (hi - lo) * rng.random((n, hw))).astype(np.float32)
    d[rng.random((n, hw)) < holes] = np.inf
    return d


def walk(n, steps, start=(-3.37, 7.21), seed=5):
    """`steps` lists of (pos (n, 3), quat (n, 4)) float32: moves of a few tenths of a metre in +x / -y, -x / +y and diagonally from
    negative x and positive y, the yaw in another quadrant at every step and env, small pitch and roll."""
    rng = np.random.default_rng(seed)
    moves = [(0.0, 0.0), (0.31, -0.27), (-0.58, 0.0), (0.27, 0.33), (-0.26, -0.52), (0.0, 0.41)]
    p = np.array([[start[0] + 1.3 * e, start[1] - 0.9 * e, 0.3 + 0.05 * e] for e in range(n)])
    out = []
    for s in range(steps):
        p = p + np.array([*moves[s % len(moves)], 0.01])
        q = np.stack([quat(0.4 + 1.571 * (s + e), 0.05 * rng.standard_normal(), 0.05 * rng.standard_normal()) for e in range(n)])
        out.append((p.astype(np.float32), q))
    return out


def corridor(scanner=None):
    """(in front, behind): masks over the scan's columns of `ox >= 0.3 and |oy| <= 0.3` (91 columns) and of `ox < -0.2`."""
    rx, ry = elevation.scan_offsets(scanner or RayCasterCfg(), np.float64)
    ox, oy = np.meshgrid(rx, ry)                       # column i * nx + j: i over ray_y, j over ray_x
    return ((ox >= 0.3 - 1e-6) & (np.abs(oy) <= 0.3 + 1e-6)).reshape(-1), (ox < -0.2 - 1e-6).reshape(-1)
