"""Float64 numpy restatement of the rover's depth camera (test infrastructure, independent of the HIP code).

* ``ray_dirs_camera``: unit ray through each pixel centre in the USD camera frame (x right, y up, looking along -z)
* ``camera_pose``:     optical centre and camera -> world rotation from the state's position and (w, x, y, z) quaternion
* ``cast``:            exact first hit of each ray with the heightfield's triangle mesh (cells split along the (i, j) - (i+1, j+1)
                       diagonal, the mesh of ``oracle.mesh_raycast.heightfield_mesh``) by a cell DDA, plus the ray's clearance:
                       the smallest vertical gap ray - surface before the hit (over the whole march for a miss)
* ``cast_brute``:      the same depth by brute force, every ray against the mesh's triangle list (Moller-Trumbore): the oracle that
                       shares no algorithm with ``cast`` or the HIP kernel

A miss (the ray leaves the x-y extent, climbs above the highest node or passes the far clip) is +inf; hits nearer than the near
clip do not count.  The ray starts on one side of the surface (the side of its first point over the terrain, touching counts as
above, and a ray entering the range through the terrain's maximum height is above) and the hit is the first point where it
reaches the other.
"""
from __future__ import annotations

import numpy as np


def quat_to_mat(q) -> np.ndarray:
    """(..., 4) (w, x, y, z) -> (..., 3, 3), normalised first."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def focal_px(cam) -> tuple:
    fx = cam.width * cam.focal_length / cam.horizontal_aperture
    fy = fx if cam.vertical_aperture is None else cam.height * cam.focal_length / cam.vertical_aperture
    return fx, fy


def ray_dirs_camera(cam) -> np.ndarray:
    """(height, width, 3) unit directions in the camera frame; pixel (u, v) = (column, row), row 0 at the top."""
    fx, fy = focal_px(cam)
    u = np.arange(cam.width, dtype=np.float64) + 0.5 - 0.5 * cam.width
    v = np.arange(cam.height, dtype=np.float64) + 0.5 - 0.5 * cam.height
    U, V = np.meshgrid(u / fx, -v / fy, indexing="xy")
    d = np.stack([U, V, -np.ones_like(U)], -1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def ray_dirs_body(cam) -> np.ndarray:
    return ray_dirs_camera(cam) @ quat_to_mat(cam.orientation).T


def camera_pose(cam, pos, quat):
    """(N, 3) optical centres and (N, 3, 3) camera -> world rotations for body positions ``pos`` and quaternions ``quat``."""
    Rb = quat_to_mat(np.asarray(quat, dtype=np.float64))
    o = np.asarray(pos, dtype=np.float64) + Rb @ np.asarray(cam.position, dtype=np.float64)
    return o, Rb @ quat_to_mat(cam.orientation)


def camera_rays(cam, pos, quat):
    """(N, 3) origins and (N, height, width, 3) world directions."""
    o, R = camera_pose(cam, pos, quat)
    d = np.einsum("nij,hwj->nhwi", R, ray_dirs_camera(cam))
    return o, d


def cast(height, res, min_x, min_y, origins, dirs, near=0.01, far=1e6):
    """First hit of rays ``origins`` (R, 3) + t ``dirs`` (R, 3) (unit) with the triangle mesh of ``height`` (H, W), row = y.
    Returns (depth (R,), clearance (R,)), float64."""
    h = np.asarray(height, dtype=np.float64)
    H, W = h.shape
    o = np.asarray(origins, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float64)
    R = o.shape[0]
    gox, goy = (o[:, 0] - min_x) / res, (o[:, 1] - min_y) / res
    gdx, gdy = d[:, 0] / res, d[:, 1] / res
    oz, dz = o[:, 2], d[:, 2]
    zmax = float(h.max())
    with np.errstate(divide="ignore", invalid="ignore"):
        t_lo = np.full(R, float(near))
        t_hi = np.full(R, float(far))
        miss = np.zeros(R, bool)
        for g0, gd, hi in ((gox, gdx, W - 1.0), (goy, gdy, H - 1.0)):
            par = gd == 0
            a, b = -g0 / gd, (hi - g0) / gd
            t_lo = np.where(par, t_lo, np.maximum(t_lo, np.minimum(a, b)))
            t_hi = np.where(par, t_hi, np.minimum(t_hi, np.maximum(a, b)))
            miss |= par & ~((g0 >= 0) & (g0 <= hi))
        tz = (zmax - oz) / dz
        t_hi = np.where(dz > 0, np.minimum(t_hi, tz), t_hi)
        from_top = (dz < 0) & (tz >= t_lo)         # enters through the top: above the surface before t_lo
        t_lo = np.where(dz < 0, np.maximum(t_lo, tz), t_lo)
        miss |= (dz == 0) & (oz > zmax)
        miss |= ~(t_lo <= t_hi)
    depth = np.full(R, np.inf)
    clear = np.full(R, np.inf)
    act = np.nonzero(~miss)[0]
    sx, sy = np.where(gdx > 0, 1, -1), np.where(gdy > 0, 1, -1)
    ix = np.clip(np.floor(gox + t_lo * gdx), 0, W - 2).astype(np.int64)
    iy = np.clip(np.floor(goy + t_lo * gdy), 0, H - 2).astype(np.int64)
    t = t_lo.copy()
    above = np.zeros(R, bool)
    first = np.ones(R, bool)
    while act.size:
        a_ = act
        ux, uy = (sx[a_] > 0).astype(np.float64), (sy[a_] > 0).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            tx = np.where(gdx[a_] == 0, np.inf, (ix[a_] + ux - gox[a_]) / gdx[a_])
            ty = np.where(gdy[a_] == 0, np.inf, (iy[a_] + uy - goy[a_]) / gdy[a_])
        ta = t[a_]
        tc = np.maximum(np.minimum(np.minimum(tx, ty), t_hi[a_]), ta)
        fx0, fy0 = gox[a_] - ix[a_], goy[a_] - iy[a_]
        h00 = h[iy[a_], ix[a_]]
        h01 = h[iy[a_], ix[a_] + 1]
        h10 = h[iy[a_] + 1, ix[a_]]
        h11 = h[iy[a_] + 1, ix[a_] + 1]

        def gap(tt, lower):
            ca = np.where(lower, h01 - h00, h11 - h10)
            cb = np.where(lower, h11 - h01, h10 - h00)
            return oz[a_] + tt * dz[a_] - (h00 + (fx0 + tt * gdx[a_]) * ca + (fy0 + tt * gdy[a_]) * cb)

        e0, de = fx0 - fy0, gdx[a_] - gdy[a_]
        ea, eb = e0 + ta * de, e0 + tc * de
        split = (ea >= 0) != (eb >= 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            tm = np.where(split, np.clip(-e0 / de, ta, tc), tc)
        lowerA = np.where(split, eb < 0, ea + eb >= 0)
        g_a = gap(ta, lowerA)
        g_m = gap(tm, lowerA)
        g_m2 = gap(tm, ~lowerA)
        g_c = np.where(split, gap(tc, ~lowerA), g_m)
        f = first[a_]
        above[a_] = np.where(f, from_top[a_] | (g_a >= 0), above[a_])
        first[a_] = False
        ab = above[a_]

        def crossed(g):
            return np.where(ab, g <= 0, g > 0)

        hit_a, hit_m = crossed(g_a), crossed(g_m)
        hit_c = np.where(split, crossed(g_m2) | crossed(g_c), False)
        with np.errstate(divide="ignore", invalid="ignore"):
            t_m = ta + (tm - ta) * g_a / (g_a - g_m)
            # B piece: its own plane's values at tm and tc (equal to A's at tm up to rounding: the mesh is continuous)
            t_c = np.where(crossed(g_m2), tm, tm + (tc - tm) * g_m2 / (g_m2 - g_c))
        hit = hit_a | hit_m | hit_c
        dep = np.where(hit_a, ta, np.where(hit_m, t_m, t_c))
        # clearance before the hit: gap values at the piece ends passed without a crossing, measured on the side the ray
        # started on (a ray from below has negative gaps: its clearance is the smallest of their magnitudes)
        sd = np.where(ab, 1.0, -1.0)
        c_a, c_m, c_m2, c_c = sd * g_a, sd * g_m, sd * g_m2, sd * g_c
        cl = np.where(hit_a, np.inf, np.where(hit_m, c_a, np.minimum(c_a, np.where(split, np.minimum(c_m, c_m2), c_m))))
        cl = np.where(hit, cl, np.minimum(np.minimum(c_a, c_m), np.where(split, np.minimum(c_m2, c_c), c_m)))
        clear[a_] = np.minimum(clear[a_], cl)
        depth[a_[hit]] = dep[hit]
        step_x = tx <= ty
        nix = ix[a_] + np.where(step_x, sx[a_], 0)
        niy = iy[a_] + np.where(step_x, 0, sy[a_])
        out = (tc >= t_hi[a_]) | (nix < 0) | (niy < 0) | (nix > W - 2) | (niy > H - 2)
        ix[a_], iy[a_], t[a_] = nix, niy, tc
        act = a_[~hit & ~out]
    return depth, clear


def _slab(o, d, lo, hi, t0, t1):
    """Entry / exit t of rays o + t d (..., 3) through boxes [lo, hi] (..., 3), clipped to [t0, t1]; an axis the ray does not move
    along admits every t when the origin lies in the slab (boundary included) and none otherwise."""
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = (lo - o) / d, (hi - o) / d
    par = d == 0
    inside = (o >= lo) & (o <= hi)
    ta = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(a, b))
    tb = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(a, b))
    return np.maximum(ta.max(-1), t0), np.minimum(tb.min(-1), t1)


def cast_brute(height, res, min_x, min_y, origins, dirs, near=0.01, far=1e6, block=8):
    """Depth of rays ``origins`` (R, 3) + t ``dirs`` (R, 3) (unit): the smallest t in [near, far] at which the ray meets a
    triangle of ``oracle.mesh_raycast.heightfield_mesh`` (Moller-Trumbore, float64), +inf where there is none.

    An oracle independent of ``cast``: no grid walk and no per-cell diagonal logic, only the mesh's triangle list.  The one
    culling is conservative: a triangle is tested only when the ray passes through the box of its ``block`` x ``block`` cell
    block and then of its cell (x-y extent of the nodes, z from their minimum to their maximum, widened by a hair)."""
    from oracle.mesh_raycast import heightfield_mesh
    h = np.asarray(height, dtype=np.float64)
    H, W = h.shape
    V, F = heightfield_mesh(h, res, min_x, min_y)
    ncell = (H - 1) * (W - 1)
    tri = V[F]                                               # (2 * ncell, 3, 3): cell k's triangles are k and ncell + k
    # cell boxes, then block boxes over them
    lo_c, hi_c = np.minimum(tri[:ncell].min(1), tri[ncell:].min(1)), np.maximum(tri[:ncell].max(1), tri[ncell:].max(1))
    pad = 1e-9 * (1.0 + np.abs(V).max())
    lo_c, hi_c = lo_c - pad, hi_c + pad
    ci, cj = np.divmod(np.arange(ncell), W - 1)
    bid = (ci // block) * ((W - 2) // block + 1) + cj // block
    nb = int(bid.max()) + 1
    lo_b, hi_b = np.full((nb, 3), np.inf), np.full((nb, 3), -np.inf)
    np.minimum.at(lo_b, bid, lo_c)
    np.maximum.at(hi_b, bid, hi_c)
    cells_of = np.split(np.argsort(bid, kind="stable"), np.cumsum(np.bincount(bid, minlength=nb))[:-1])
    o = np.asarray(origins, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float64)
    out = np.full(o.shape[0], np.inf)
    for r in range(o.shape[0]):
        ta, tb = _slab(o[r], d[r], lo_b, hi_b, near, far)
        blocks = np.nonzero(ta <= tb)[0]
        if blocks.size == 0:
            continue
        cells = np.concatenate([cells_of[b] for b in blocks])
        ta, tb = _slab(o[r], d[r], lo_c[cells], hi_c[cells], near, far)
        cells = cells[ta <= tb]
        if cells.size == 0:
            continue
        t3 = tri[np.concatenate([cells, cells + ncell])]
        v0 = t3[:, 0]
        e1, e2 = t3[:, 1] - v0, t3[:, 2] - v0
        p = np.cross(d[r], e2)
        det = np.einsum("ij,ij->i", e1, p)
        ok = det != 0.0                                      # 0: the ray runs in the triangle's plane (touching only)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            s = o[r] - v0
            u = np.einsum("ij,ij->i", s, p) * inv
            q = np.cross(s, e1)
            v = (q @ d[r]) * inv
            t = np.einsum("ij,ij->i", e2, q) * inv
            eps = 1e-12
            ok &= (u >= -eps) & (v >= -eps) & (u + v <= 1.0 + eps) & (t >= near) & (t <= far)
        if ok.any():
            out[r] = t[ok].min()
    return out


def render(cam, height, res, min_x, min_y, pos, quat):
    """(N, cam.height, cam.width) depth and clearance images for body poses ``pos`` (N, 3), ``quat`` (N, 4)."""
    o, d = camera_rays(cam, pos, quat)
    N = o.shape[0]
    rays = d.reshape(N, -1, 3)
    org = np.repeat(o[:, None, :], rays.shape[1], 1)
    dep, cl = cast(height, res, min_x, min_y, org.reshape(-1, 3), rays.reshape(-1, 3), cam.near_clip, cam.far_clip)
    return dep.reshape(N, cam.height, cam.width), cl.reshape(N, cam.height, cam.width)
