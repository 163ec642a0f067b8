"""Depth camera (RoverEnvCamera): configuration, geometry of the reference's mount and lens, the float64 reference camera against
closed forms, and the C ABI's struct.  CPU only."""
import ctypes as C
import math

import numpy as np
import pytest

from camera_reference import camera_rays, focal_px, quat_to_mat, ray_dirs_body, render
from isaac_rover_orbit_amd.cfg import AAURoverCameraEnvCfg, CameraCfg, RoverEnvCfg


def test_defaults_are_the_reference_constants():
    c = CameraCfg()      # rover_camera_env.py:44-62
    assert (c.width, c.height) == (160, 90)
    assert (c.focal_length, c.horizontal_aperture, c.vertical_aperture) == (2.12, 6.055, None)
    assert c.position == (-0.151, 0.0, 0.73428)
    assert c.orientation == (0.64086, 0.29884, -0.29884, -0.64086)
    assert (c.near_clip, c.far_clip, c.every_n_steps) == (0.01, 1000000.0, 1)
    assert RoverEnvCfg().camera is None
    assert AAURoverCameraEnvCfg().camera == CameraCfg()


def test_focal_length_and_fields_of_view():
    fx, fy = CameraCfg().focal_px
    assert fx == fy
    assert abs(fx - 56.020) < 5e-4
    assert abs(2 * math.degrees(math.atan(80 / fx)) - 110.0) < 0.01
    assert abs(2 * math.degrees(math.atan(45 / fy)) - 77.55) < 0.01
    _, fy70 = CameraCfg(vertical_aperture=2.968879962).focal_px
    assert abs(2 * math.degrees(math.atan(45 / fy70)) - 70.0) < 1e-6


def test_optical_axis_and_corner_rays():
    c = CameraCfg()
    q = np.array(c.orientation)
    assert abs(np.dot(q, q) - 1.0000138) < 1e-7          # normalised before use
    R = quat_to_mat(q)
    axis = R @ [0, 0, -1]
    assert np.allclose(axis, [0.7661, 0.0, -0.6428], atol=1e-4)
    assert np.allclose(R @ [1, 0, 0], [0, -1, 0], atol=1e-4)      # image-right = -y_body
    th = math.radians(40.0)
    fwd, right, up = np.array([math.cos(th), 0, -math.sin(th)]), np.array([0, -1.0, 0]), np.array([math.sin(th), 0, math.cos(th)])
    f = c.width * c.focal_length / c.horizontal_aperture
    d = ray_dirs_body(c)
    for v, u in ((0, 0), (0, 159), (89, 0), (89, 159)):
        x, y = (u + 0.5 - 80) / f, -(v + 0.5 - 45) / f
        ref = fwd + x * right + y * up
        assert np.allclose(d[v, u], ref / np.linalg.norm(ref), atol=1e-4), (u, v)


def _plane_closed_form(cam, o, d, a, b, c, extent):
    t = (a * o[0] + b * o[1] + c - o[2]) / (d[..., 2] - a * d[..., 0] - b * d[..., 1])
    p = o + t[..., None] * d
    inside = (t >= cam.near_clip) & (p[..., 0] >= extent[0]) & (p[..., 0] <= extent[1]) & (p[..., 1] >= extent[2]) & (p[..., 1] <= extent[3])
    return np.where(inside, t, np.inf)


@pytest.mark.parametrize("a,b,c", [(0.0, 0.0, 0.0), (0.0, 0.0, -1.25), (0.12, -0.07, 0.3), (-0.2, 0.15, 1.0)])
def test_reference_camera_equals_the_closed_form_on_planes(a, b, c):
    cam = CameraCfg()
    H, W, res, x0, y0 = 160, 200, 0.05, -3.0, 2.0
    X, Y = np.meshgrid(x0 + res * np.arange(W), y0 + res * np.arange(H))
    h = a * X + b * Y + c
    rng = np.random.default_rng(3)
    poses = []
    for k in range(4):
        px, py = x0 + rng.uniform(1, 9), y0 + rng.uniform(1, 7)
        yaw, pitch, roll = rng.uniform(-math.pi, math.pi), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)
        cy, sy, cp, sp, cr_, sr = (math.cos(yaw / 2), math.sin(yaw / 2), math.cos(pitch / 2), math.sin(pitch / 2),
                                   math.cos(roll / 2), math.sin(roll / 2))
        q = [cr_ * cp * cy + sr * sp * sy, sr * cp * cy - cr_ * sp * sy, cr_ * sp * cy + sr * cp * sy, cr_ * cp * sy - sr * sp * cy]
        poses.append(([px, py, a * px + b * py + c + 0.2], q))
    pos, quat = np.array([p for p, _ in poses]), np.array([q for _, q in poses])
    dep, _ = render(cam, h, res, x0, y0, pos, quat)
    o, d = camera_rays(cam, pos, quat)
    extent = (x0, x0 + (W - 1) * res, y0, y0 + (H - 1) * res)
    for k in range(len(poses)):
        exp = _plane_closed_form(cam, o[k], d[k], a, b, c, extent)
        fin = np.isfinite(exp)
        assert fin.any() and (~fin).any()
        assert (np.isfinite(dep[k]) == fin).all()
        assert np.allclose(dep[k][fin], exp[fin], rtol=1e-9, atol=0)


def test_native_default_config_matches_the_cfg():
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    assert lib.rover_camera_config_bytes() == C.sizeof(_lib.CameraConfig)
    native, mine = _lib.default_camera_config(), CameraCfg().to_native()
    for name, _ in _lib.CameraConfig._fields_:
        a, b = getattr(native, name), getattr(mine, name)
        if hasattr(a, "_length_"):
            a, b = list(a), list(b)
        assert a == b, name


def test_native_entry_points_reject_bad_calls():
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    cfg = _lib.default_camera_config()
    assert lib.rover_camera_workspace_bytes(None, C.byref(cfg)) == 0
    assert lib.rover_camera_prepare(None, C.byref(cfg), None, 0, None) == 1
    assert lib.rover_camera_render(None, C.byref(cfg), None, None, None) == 1


@pytest.mark.parametrize("field,value", [("width", 0), ("height", -1), ("focal_length", 0.0), ("horizontal_aperture", -1.0),
                                         ("vertical_aperture", 0.0), ("near_clip", 2e6), ("near_clip", -0.1),
                                         ("every_n_steps", 0), ("orientation", (0.0, 0.0, 0.0, 0.0)),
                                         ("focal_length", math.inf), ("focal_length", math.nan), ("focal_length", 1e39),
                                         ("horizontal_aperture", math.inf), ("horizontal_aperture", math.nan),
                                         ("vertical_aperture", math.inf), ("vertical_aperture", math.nan), ("far_clip", math.nan),
                                         ("near_clip", math.nan), ("position", (0.0, math.nan, 0.7)), ("position", (math.inf, 0.0, 0.7)),
                                         ("orientation", (math.inf, 0.0, 0.0, 0.0)), ("orientation", (1.0, math.nan, 0.0, 0.0))])
def test_validate_rejects_bad_values(field, value):
    cam = CameraCfg()
    setattr(cam, field, value)
    with pytest.raises(ValueError):
        cam.validate()
    cfg = RoverEnvCfg()
    cfg.camera = cam
    with pytest.raises(ValueError):
        cfg.validate()


def test_validate_accepts_an_infinite_far_clip_and_a_scaled_quaternion():
    cam = CameraCfg(far_clip=math.inf, orientation=tuple(4 * q for q in CameraCfg().orientation), near_clip=0.0)
    cam.validate()
    assert cam.to_native().far_clip == math.inf


def test_register_default_tasks_registers_the_camera_env():
    from isaac_rover_orbit_amd import compat
    compat.register_default_tasks()
    spec = compat.gym_api().spec("RoverCamera-v0")
    assert spec.entry_point == "isaac_rover_orbit_amd.envs:RoverEnvCamera"
    assert spec.kwargs["env_cfg_entry_point"] is AAURoverCameraEnvCfg


# ---- the DDA reference (cast) against the brute-force mesh oracle (cast_brute): the two share no algorithm
def _terrain(kind):
    """(height, resolution, min_x, min_y): small non-planar terrains on which the cell diagonal matters."""
    if kind == "normal":
        h = np.random.default_rng(11).normal(0.0, 0.3, (37, 53))
        return h, 0.1, -1.0, 2.0
    i, j = np.meshgrid(np.arange(29), np.arange(41), indexing="ij")
    if kind == "checker":         # diagonal nodes low, off-diagonal nodes high: the other split turns every valley into a ridge
        return 0.4 * ((i + j) % 2), 0.07, 0.5, -3.0
    if kind == "ridge":           # a triangle wave along (1, 1): slopes across the diagonal
        return 0.15 * np.abs((i + j) % 6 - 3.0), 0.05, -2.0, -1.5
    if kind == "sawtooth":        # ridges along the diagonal that fall the other way each period
        return 0.5 * (((j - i) % 5) / 5.0) - 0.1 * i / 28, 0.1, 3.0, 0.25
    raise ValueError(kind)


def _agree(h, res, x0, y0, o, d, near=0.01, far=1e6, grazing_share=0.002):
    """cast == cast_brute on every ray (hit / miss and depth to 1e-9 relative); only rays that graze the mesh (clearance
    <= 1e-9 m), at most ``grazing_share`` of them, may differ.  Returns the depths."""
    from camera_reference import cast, cast_brute
    a, clear = cast(h, res, x0, y0, o, d, near, far)
    b = cast_brute(h, res, x0, y0, o, d, near, far)
    same = np.isfinite(a) == np.isfinite(b)
    fin = same & np.isfinite(a)
    same[fin] = np.abs(a[fin] - b[fin]) <= 1e-9 * b[fin] + 1e-12
    bad = np.nonzero(~same)[0]
    assert (clear[bad] <= 1e-9).all(), f"{bad.size} rays differ, e.g. ray {bad[0] if bad.size else None}"
    assert bad.size <= max(2, int(grazing_share * a.size))
    return b


def _unit(d):
    d = np.asarray(d, dtype=np.float64)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _extent(h, res, x0, y0):
    H, W = h.shape
    return x0, x0 + (W - 1) * res, y0, y0 + (H - 1) * res


def _surface_at(h, res, x0, y0, x, y):
    from camera_reference import cast
    o = np.stack([x, y, np.full_like(x, float(h.max()) + 5.0)], 1)
    d = np.tile([0.0, 0.0, -1.0], (len(x), 1))
    t, _ = cast(h, res, x0, y0, o, d, 0.0)
    return o[:, 2] - t


@pytest.mark.parametrize("kind", ["normal", "checker", "ridge", "sawtooth"])
def test_cast_matches_brute_force_from_inside(kind):
    h, res, x0, y0 = _terrain(kind)
    xa, xb, ya, yb = _extent(h, res, x0, y0)
    rng = np.random.default_rng(1)
    R = 600
    o = np.stack([rng.uniform(xa, xb, R), rng.uniform(ya, yb, R), np.zeros(R)], 1)
    o[:, 2] = _surface_at(h, res, x0, y0, o[:, 0], o[:, 1]) + rng.uniform(0.05, 1.5, R)
    d = _unit(rng.normal(size=(R, 3)) + [0.0, 0.0, -0.4])
    dep = _agree(h, res, x0, y0, o, d)
    assert 0.3 < np.isfinite(dep).mean() < 0.95


@pytest.mark.parametrize("kind", ["normal", "checker", "sawtooth"])
def test_cast_matches_brute_force_from_outside_the_extent(kind):
    """Cameras beyond each side and each corner of the x-y extent, looking in (slightly down) and across."""
    h, res, x0, y0 = _terrain(kind)
    xa, xb, ya, yb = _extent(h, res, x0, y0)
    xm, ym = 0.5 * (xa + xb), 0.5 * (ya + yb)
    rng = np.random.default_rng(2)
    top = float(h.max())
    n_hit = 0
    for px, py in ((xa - 1.0, ym), (xb + 1.0, ym), (xm, ya - 1.0), (xm, yb + 1.0),
                   (xa - 0.7, ya - 0.4), (xb + 0.3, yb + 0.9), (xa - 0.5, yb + 0.5), (xb + 0.8, ya - 0.2)):
        o = np.tile([px, py, top + 0.4], (300, 1))
        tgt = np.stack([rng.uniform(xa, xb, 300), rng.uniform(ya, yb, 300), rng.uniform(-0.6, top, 300)], 1)
        d = _unit(tgt - o)
        d[:40] = _unit(rng.normal(size=(40, 3)))            # some looking anywhere, away from the terrain included
        dep = _agree(h, res, x0, y0, o, d)
        n_hit += int(np.isfinite(dep).sum())
    assert n_hit > 1000


@pytest.mark.parametrize("kind", ["normal", "ridge"])
def test_cast_matches_brute_force_from_below_the_surface(kind):
    h, res, x0, y0 = _terrain(kind)
    xa, xb, ya, yb = _extent(h, res, x0, y0)
    rng = np.random.default_rng(3)
    R = 500
    o = np.stack([rng.uniform(xa + 0.2, xb - 0.2, R), rng.uniform(ya + 0.2, yb - 0.2, R), np.zeros(R)], 1)
    o[:, 2] = _surface_at(h, res, x0, y0, o[:, 0], o[:, 1]) - rng.uniform(0.02, 0.5, R)
    d = _unit(rng.normal(size=(R, 3)))
    d[:50] = (0.0, 0.0, 1.0)
    dep = _agree(h, res, x0, y0, o, d)
    assert np.isfinite(dep[:50]).all()                      # a buried camera looking straight up sees the surface above it
    assert 0.3 < np.isfinite(dep[50:]).mean() < 1.0


@pytest.mark.parametrize("near,far", [(0.5, 1e6), (2.0, 1e6), (0.01, 3.0), (0.5, 3.0)])
def test_cast_matches_brute_force_with_clipping(near, far):
    h, res, x0, y0 = _terrain("normal")
    xa, xb, ya, yb = _extent(h, res, x0, y0)
    rng = np.random.default_rng(4)
    R = 600
    o = np.stack([rng.uniform(xa, xb, R), rng.uniform(ya, yb, R), np.zeros(R)], 1)
    o[:, 2] = _surface_at(h, res, x0, y0, o[:, 0], o[:, 1]) + rng.uniform(-0.3, 1.2, R)
    d = _unit(rng.normal(size=(R, 3)) + [0.0, 0.0, -0.3])
    dep = _agree(h, res, x0, y0, o, d, near, far)
    fin = np.isfinite(dep)
    assert fin.any() and (dep[fin] >= near).all() and (dep[fin] <= far).all()
    from camera_reference import cast_brute
    unclipped = cast_brute(h, res, x0, y0, o, d, 0.0, 1e6)
    assert (np.isfinite(unclipped) & ~fin).any()            # the clip range removed hits


@pytest.mark.parametrize("kind", ["normal", "checker", "sawtooth"])
def test_cast_matches_brute_force_on_axis_aligned_rays(kind):
    """Rays with exact zero components (dx = 0, dy = 0, dz = 0 and two of them at once), from on and off the grid lines,
    below, at and above the highest node."""
    h, res, x0, y0 = _terrain(kind)
    H, W = h.shape
    xa, xb, ya, yb = _extent(h, res, x0, y0)
    top = float(h.max())
    dirs = _unit([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, -1], [0, 0, 1], [1, 0, -0.3], [-1, 0, -0.7],
                  [0, 1, -0.2], [0, -1, -1.5], [1, 1, 0], [2, -1, 0], [1, 1, -0.4], [0, 0.5, 1.0]])
    org = []
    for i, j in ((0, 0), (H - 1, W - 1), (H // 2, W // 3), (7, 8), (H - 2, 1)):
        for fx, fy in ((0.0, 0.0), (0.5, 0.0), (0.0, 0.25), (0.3, 0.7)):
            x, y = x0 + (j + fx) * res, y0 + (i + fy) * res
            x, y = min(x, xb), min(y, yb)
            for z in (top + 0.5, top, 0.5 * (top + h.min()) + 0.0123, h.min() - 0.2):
                org.append((x, y, z))
    org += [(xa - 0.3, y0 + 3 * res, top - 0.1234), (xb + 0.2, y0 + 5 * res, 0.0), (x0 + 4 * res, ya - 0.5, 0.0)]
    org = np.array(org)
    o = np.repeat(org, len(dirs), 0)
    d = np.tile(dirs, (len(org), 1))
    dep = _agree(h, res, x0, y0, o, d, grazing_share=0.01)     # horizontal rays at the height of the peaks touch them
    assert np.isfinite(dep).sum() > 200
