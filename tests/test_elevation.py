"""The rolling elevation map's CPU side (include/rover_elevation.h, isaac_rover_orbit_amd.elevation): TorchElevationMap, the
specification, against a hand-written loop on Python floats; a plane seen through the real camera; the scroll rule; memory behind
the rover; every refusal of the library (no GPU needed: the arguments are checked before the device is looked at) and of the cfg
classes; the kernels' resources from the code object; the example's flags."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import elevation_cases as cases
from isaac_rover_orbit_amd import _lib, elevation
from isaac_rover_orbit_amd.cfg import CameraCfg, ElevationMapCfg, RayCasterCfg, RoverEnvCfg
from isaac_rover_orbit_amd.elevation import TorchElevationMap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32(x: float) -> float:
    """A Python float rounded to fp32.  +, -, *, / and sqrt of fp32 values evaluated in double and rounded once more give the
    correctly rounded fp32 result (double carries more than 2 * 24 + 2 bits), so the loop below is fp32 arithmetic."""
    return C.c_float(x).value


def _cell(v, inv_cell):
    return int(min(max(math.floor(f32(v * inv_cell)), -2 ** 30), 2 ** 30))


def by_hand(c, rays, ray_x, ray_y, H, W, mp, origin, depth, pos, quat, reset):
    """One env through the header's eight steps on Python floats.  `mp`: G x G nested lists, changed in place.  Returns (origin,
    scan, known)."""
    G, nan = c.grid, math.nan
    px, py, pz = pos
    w, x, y, z = quat
    unknown = ([c.unknown_value] * (len(ray_x) * len(ray_y)), [0] * (len(ray_x) * len(ray_y)))
    if reset:
        for row in mp:
            row[:] = [nan] * G
    if not all(math.isfinite(v) for v in (*pos, *quat)):
        return origin, *unknown
    cx, cy = _cell(px, c.inv_cell), _cell(py, c.inv_cell)
    lo, olo = (cx - G // 2, cy - G // 2), (origin[0] - G // 2, origin[1] - G // 2)
    for sy in range(G):
        for sx in range(G):
            new = (lo[0] + ((sx - lo[0]) % G), lo[1] + ((sy - lo[1]) % G))
            old = (olo[0] + ((sx - olo[0]) % G), olo[1] + ((sy - olo[1]) % G))
            if new != old:
                mp[sy][sx] = nan
    frame = {}
    if depth is not None:
        R = [f32(1 - f32(2 * f32(f32(y * y) + f32(z * z)))), f32(2 * f32(f32(x * y) - f32(w * z))), f32(2 * f32(f32(x * z) + f32(w * y))),
             f32(2 * f32(f32(x * y) + f32(w * z))), f32(1 - f32(2 * f32(f32(x * x) + f32(z * z)))), f32(2 * f32(f32(y * z) - f32(w * x))),
             f32(2 * f32(f32(x * z) - f32(w * y))), f32(2 * f32(f32(y * z) + f32(w * x))), f32(1 - f32(2 * f32(f32(x * x) + f32(y * y))))]
        for k in range(H * W):
            d = depth[k]
            if not (math.isfinite(d) and c.range_min <= d <= c.range_max):
                continue
            b = [f32(c.mount_pos[i] + f32(d * rays[k][i])) for i in range(3)]
            p = [f32(o + f32(f32(f32(R[3 * r] * b[0]) + f32(R[3 * r + 1] * b[1])) + f32(R[3 * r + 2] * b[2]))) for r, o in enumerate(pos)]
            if not all(math.isfinite(v) for v in p):
                continue
            gx, gy = _cell(p[0], c.inv_cell), _cell(p[1], c.inv_cell)
            if not (lo[0] <= gx < lo[0] + G and lo[1] <= gy < lo[1] + G):
                continue
            key = (gy % G, gx % G)
            frame[key] = max(frame.get(key, -math.inf), p[2])
    for (sy, sx), f in frame.items():
        old = mp[sy][sx]
        mp[sy][sx] = f if (math.isnan(old) or c.alpha == 1.0) else f32(old + f32(c.alpha * f32(f - old)))
    a = f32(1 - f32(2 * f32(f32(y * y) + f32(z * z))))
    b = f32(2 * f32(f32(w * z) + f32(x * y)))
    inv = f32(1 / f32(math.sqrt(f32(f32(a * a) + f32(b * b)))))
    cyaw, syaw = f32(a * inv), f32(b * inv)
    scan, known = [], []
    for oy in ray_y:
        for ox in ray_x:
            sx_ = f32(px + f32(f32(cyaw * ox) - f32(syaw * oy)))
            sy_ = f32(py + f32(f32(syaw * ox) + f32(cyaw * oy)))
            gx, gy = _cell(sx_, c.inv_cell), _cell(sy_, c.inv_cell)
            h = mp[gy % G][gx % G] if (lo[0] <= gx < lo[0] + G and lo[1] <= gy < lo[1] + G) else nan
            known.append(0 if math.isnan(h) else 1)
            scan.append(c.unknown_value if math.isnan(h) else f32(f32(pz - h) - c.height_offset))
    return (cx, cy), scan, known


@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_spec_against_a_hand_written_loop(alpha):
    """3 envs, 12 x 16 image, G = 16, three steps that scroll, fuse and reset; the last without a frame."""
    n, H, W, G = 3, 12, 16, 16
    ecfg, cam, sc = cases.cfgs(H, W, G, cell=0.25, alpha=alpha, unknown_value=-7.5)
    spec = TorchElevationMap(ecfg, cam, sc, n)
    c = spec.cfg
    rays, rx, ry = [[float(v) for v in r] for r in spec.rays], [float(v) for v in spec.ray_x], [float(v) for v in spec.ray_y]
    maps = [[[math.nan] * G for _ in range(G)] for _ in range(n)]
    origins = [(0, 0)] * n
    rng = np.random.default_rng(21)
    for s, (pos, quat) in enumerate(cases.walk(n, 3)):
        depth = cases.random_depth(rng, n, H * W, 0.4, 3.0) if s < 2 else None
        flags = np.array([0, s == 1, 0], np.uint8)
        scan, known, count = spec.update(depth, pos, quat, reset=(flags, None))
        for e in range(n):
            origins[e], hs, hk = by_hand(c, rays, rx, ry, H, W, maps[e], origins[e], None if depth is None else [float(v) for v in depth[e]],
                                         [float(v) for v in pos[e]], [float(v) for v in quat[e]], bool(flags[e]))
            assert tuple(spec.origin[e]) == origins[e]
            assert np.array_equal(spec.map[e].view(np.int32), np.array(maps[e], np.float32).view(np.int32)), (s, e)
            assert np.array_equal(scan[e].view(np.int32), np.array(hs, np.float32).view(np.int32)) and known[e].tolist() == hk
            assert count[e] == sum(hk) > 0
    assert np.isfinite(spec.map).reshape(n, -1).sum(1).min() > 20 and scan.dtype == np.float32 and spec.map.dtype == np.float32


_PLANE_POSES = [(z, yaw) for z in (0.2, 0.3, 0.4, 0.5) for yaw in (0.0, 0.3, 0.785)]


@pytest.fixture(scope="module")
def plane_frames():
    """Depth of a terrain at height c through the default camera at the twelve poses, from the camera's float64 reference."""
    from camera_reference import render
    c, cam = 0.37, CameraCfg()
    pos = np.array([[51.23 + 0.7 * k, 48.91 - 0.4 * k, c + z] for k, (z, _) in enumerate(_PLANE_POSES)])
    quat = np.stack([[math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)] for _, yaw in _PLANE_POSES])
    depth, _ = render(cam, np.full((1024, 1024), c), 0.1, 0.0, 0.0, pos, quat)
    return c, cam, pos, quat, depth.reshape(len(pos), -1)


@pytest.mark.parametrize("float64", [True, False])
def test_a_plane_through_the_real_camera(plane_frames, float64):
    """ONE frame fills the corridor in front (ox >= 0.3, |oy| <= 0.3: 91 columns) at all twelve poses and nothing behind
    (ox < -0.2); a known column reads pos.z - c - height_offset: to 1e-12 in float64 (the ray table unrounded), within 8 ulp of
    5 m (the range cap) in fp32."""
    c, cam, pos, quat, depth = plane_frames
    sc = RayCasterCfg()
    front, behind = cases.corridor(sc)
    assert front.sum() == 91
    spec = TorchElevationMap(ElevationMapCfg(), cam, sc, len(pos), float64=float64)
    p, q, d = (pos, quat, depth) if float64 else (pos.astype(np.float32), quat.astype(np.float32), depth.astype(np.float32))
    scan, known, count = spec.update(d, p, q)
    known = known.astype(bool)
    assert known[:, front].all() and not known[:, behind].any() and (count == known.sum(1)).all()
    want = (p[:, 2].astype(np.float64) - c - sc.height_offset)[:, None] * np.ones_like(scan, dtype=np.float64)
    err = np.abs(scan.astype(np.float64) - want)[known].max()
    print(f"float64={float64}: {known.sum(1).min()} .. {known.sum(1).max()} known columns, largest error {err:.3e} m")
    assert scan.dtype == (np.float64 if float64 else np.float32)
    assert err <= (1e-12 if float64 else 8 * float(np.spacing(np.float32(5.0))))
    assert (scan[~known] == 0.0).all()


def _global_cells(mp, origin, G):
    lo = (int(origin[0]) - G // 2, int(origin[1]) - G // 2)
    return {(lo[0] + ((sx - lo[0]) % G), lo[1] + ((sy - lo[1]) % G)): mp[sy, sx].view(np.int32).item() for sy in range(G) for sx in range(G)}


@pytest.mark.parametrize("start, move", [((0.3, 0.3), (1, 0)), ((0.3, 0.3), (0, -1)), ((-0.3, -0.3), (3, 5)), ((-0.3, 0.55), (-7, 2)),
                                         ((-2.0, -0.5), (15, -15)), ((-2.0, -0.5), (16, 0)), ((0.3, -0.3), (0, -16)),
                                         ((10.0, -7.25), (-40, 33)), ((-0.3, -0.3), (0, 0))])
def test_scroll_keeps_exactly_the_cells_of_both_windows(start, move):
    """A random, fully known map; a move by (kx, ky) cells keeps exactly the global cells that lie in both windows, bit for bit,
    and a move of G or more on an axis clears all.  (-0.3, -0.3) lies in cell (-2, -2): floorf, where truncation gives (-1, -1);
    (-2.0, -0.5) and (10.0, -7.25) lie exactly on cell edges."""
    G, cell = 16, 0.25
    ecfg, cam, sc = cases.cfgs(12, 16, G, cell=cell)
    spec = TorchElevationMap(ecfg, cam, sc, 1)
    q = cases.quat(0.7)[None]
    p0 = np.array([[start[0], start[1], 0.3]], np.float32)
    spec.update(None, p0, q)
    c0 = (math.floor(start[0] / cell), math.floor(start[1] / cell))
    assert tuple(spec.origin[0]) == c0
    if start == (-0.3, -0.3):
        assert c0 == (-2, -2)
    spec.map[...] = np.random.default_rng(1).standard_normal((1, G, G)).astype(np.float32)
    before = _global_cells(spec.map[0], spec.origin[0], G)
    p1 = p0 + np.array([[move[0] * cell, move[1] * cell, 0.0]], np.float32)
    spec.update(None, p1, q)
    assert tuple(spec.origin[0]) == (c0[0] + move[0], c0[1] + move[1])
    after = _global_cells(spec.map[0], spec.origin[0], G)
    nan = np.float32(np.nan).view(np.int32).item()
    assert all(v == before.get(k, nan) for k, v in after.items())
    kept = sum(k in before for k in after)
    assert kept == max(G - abs(move[0]), 0) * max(G - abs(move[1]), 0)
    assert np.isfinite(spec.map).sum() == kept


def test_the_map_remembers_what_is_now_behind_the_rover():
    """One frame, then 1.0 m ahead without a frame: the columns now behind the rover (ox in [-0.7, -0.2), |oy| <= 0.3) are known
    and read the first frame's cells."""
    cam, sc = CameraCfg(), RayCasterCfg()
    spec = TorchElevationMap(ElevationMapCfg(), cam, sc, 1)
    pos, q = np.array([[5.03, -2.07, 0.3]], np.float32), cases.quat(0.0)[None]
    _, known0, _ = spec.update(cases.plane_depth(cam, pos, q, ground=0.011), pos, q)
    first = spec.map.copy()
    ahead = pos + np.array([[1.0, 0.0, 0.0]], np.float32)
    scan, known, count = spec.update(None, ahead, q)
    ox, oy = np.meshgrid(spec.ray_x.astype(np.float64), spec.ray_y.astype(np.float64))
    back = ((ox >= -0.7 - 1e-6) & (ox < -0.2 - 1e-6) & (np.abs(oy) <= 0.3 + 1e-6)).reshape(-1)
    assert back.sum() == 35 and known[0].astype(bool)[back].all() and not known0[0].astype(bool)[back].any()
    gx = np.floor((ahead[0, 0] + ox.reshape(-1)[back].astype(np.float32)) * np.float32(10.0)).astype(int)
    gy = np.floor((ahead[0, 1] + oy.reshape(-1)[back].astype(np.float32)) * np.float32(10.0)).astype(int)
    h = first[0, gy & 63, gx & 63]
    assert np.isfinite(h).all() and np.array_equal(scan[0, back].view(np.int32), ((ahead[0, 2] - h) - np.float32(sc.height_offset)).view(np.int32))
    assert np.abs(h - 0.011).max() < 1e-5


def test_every_refusal_through_the_library():
    lib = _lib.load()
    assert lib.rover_elevation_cfg_bytes() == C.sizeof(_lib.ElevationCfg) == 44
    buf = np.zeros(8192, np.float32)
    base = buf.ctypes.data                               # never read or written: every call below is refused
    nan, inf = math.nan, math.inf
    MAP, ORG, DEP, RAY, POSE, RX, RY, SCAN, KNOWN, COUNT = (base + 4 * o for o in (0, 2048, 2304, 2560, 2816, 2880, 2912, 3072, 4096, 4160))

    def native(**kw):
        c = ElevationMapCfg(grid=16, cell=0.25).to_native((0.1, 0.0, 0.7), 0.25)
        for k, v in kw.items():
            if k == "mount_pos":
                for i in range(3):
                    c.mount_pos[i] = v[i]
            else:
                setattr(c, k, v)
        return c

    def step(cfg=None, null_cfg=False, depth=DEP, pitch=12, h=3, w=4, ray_b=RAY, pos=POSE, quat=POSE + 12, cs=1, es=7, ra=None, rb=None,
             mp=MAP, org=ORG, rx=RX, nx=5, ry=RY, ny=4, scan=SCAN, sp=20, known=KNOWN, count=COUNT, n=2):
        cfg = cfg if cfg is not None else native()
        rc = lib.rover_elevation_step(None if null_cfg else C.byref(cfg), depth, pitch, h, w, ray_b, pos, quat, cs, es, ra, rb, mp, org,
                                      rx, nx, ry, ny, scan, sp, known, count, n, None)
        return rc, lib.rover_last_error().decode()

    def scan_(cfg=None, null_cfg=False, pos=POSE, quat=POSE + 12, cs=1, es=7, mp=MAP, org=ORG, rx=RX, nx=5, ry=RY, ny=4, scan=SCAN, sp=20,
              known=KNOWN, count=COUNT, n=2, **_):
        cfg = cfg if cfg is not None else native()
        rc = lib.rover_elevation_scan(None if null_cfg else C.byref(cfg), pos, quat, cs, es, mp, org, rx, nx, ry, ny, scan, sp, known,
                                      count, n, None)
        return rc, lib.rover_last_error().decode()

    both = [
        (dict(null_cfg=True), "NULL"), (dict(pos=None), "NULL"), (dict(quat=None), "NULL"), (dict(mp=None), "NULL"),
        (dict(org=None), "NULL"), (dict(rx=None), "NULL"), (dict(ry=None), "NULL"),
        (dict(n=0), "n must"), (dict(n=-3), "n must"), (dict(nx=0), "nx and ny"), (dict(ny=-1), "nx and ny"),
        (dict(cs=0), "stride"), (dict(es=-7), "stride"),
        (dict(pos=POSE + 2), "aligned"), (dict(quat=POSE + 13), "aligned"), (dict(mp=MAP + 1), "aligned"), (dict(org=ORG + 2), "aligned"),
        (dict(rx=RX + 3), "aligned"), (dict(ry=RY + 1), "aligned"), (dict(scan=SCAN + 2), "aligned"), (dict(count=COUNT + 1), "aligned"),
        (dict(sp=19), "scan_pitch"),
        (dict(cfg=native(cell=0.0)), "cell"), (dict(cfg=native(cell=inf)), "cell"), (dict(cfg=native(cell=nan)), "cell"),
        (dict(cfg=native(inv_cell=-4.0)), "cell"), (dict(cfg=native(inv_cell=nan)), "cell"), (dict(cfg=native(inv_cell=inf)), "cell"),
        (dict(cfg=native(range_min=0.0)), "range_min"), (dict(cfg=native(range_min=-0.1)), "range_min"),
        (dict(cfg=native(range_min=nan)), "range_min"), (dict(cfg=native(range_min=inf)), "range_min"),
        (dict(cfg=native(range_min=2.0, range_max=1.0)), "range_max"), (dict(cfg=native(range_max=nan)), "range_max"),
        (dict(cfg=native(alpha=0.0)), "alpha"), (dict(cfg=native(alpha=1.5)), "alpha"), (dict(cfg=native(alpha=nan)), "alpha"),
        (dict(cfg=native(alpha=-0.5)), "alpha"),
        (dict(cfg=native(unknown_value=nan)), "unknown_value"), (dict(cfg=native(height_offset=nan)), "height_offset"),
        (dict(cfg=native(mount_pos=(0.0, inf, 0.0))), "mount_pos"), (dict(cfg=native(mount_pos=(nan, 0.0, 0.0))), "mount_pos"),
        (dict(scan=MAP + 4 * 100), "overlap"), (dict(mp=SCAN + 4 * 39), "overlap"), (dict(mp=SCAN - 4 * 511), "overlap"),
    ]
    for fn, name in ((step, "rover_elevation_step:"), (scan_, "rover_elevation_scan:")):
        for kw, text in both:
            rc, msg = fn(**kw)
            assert rc == 1 and msg.startswith(name) and text in msg, (name, kw, rc, msg)
        for kw, text in ((dict(cfg=native(grid=4)), "power of two"), (dict(cfg=native(grid=256)), "power of two"),
                         (dict(cfg=native(grid=24)), "power of two"), (dict(cfg=native(grid=0)), "power of two"),
                         (dict(nx=65, ny=64, sp=65 * 64), "4096")):
            rc, msg = fn(**kw)
            assert rc == 4 and msg.startswith(name) and text in msg, (name, kw, rc, msg)
    for kw, text in [(dict(ray_b=None), "NULL"), (dict(h=0), "height"), (dict(w=-4), "height"), (dict(pitch=11), "pitch"),
                     (dict(depth=DEP + 2), "aligned"), (dict(ray_b=RAY + 1), "aligned"),
                     (dict(depth=MAP + 4 * 500), "overlap"), (dict(mp=DEP + 4 * 23), "overlap")]:
        rc, msg = step(**kw)
        assert rc == 1 and msg.startswith("rover_elevation_step:") and text in msg, (kw, rc, msg)
    rc, msg = step(h=128, w=129, pitch=128 * 129)
    assert rc == 4 and "16384" in msg
    rc, msg = scan_(scan=None)
    assert rc == 1 and "NULL" in msg
    assert not buf.any()
    # on a host without a GPU, what is allowed gets past the argument checks and fails at the device query instead, with nothing
    # written: no depth (and then no ray_b), no scan, no known / count, range_max = +inf, +-inf unknown_value, the size limits
    import torch
    allowed = () if torch.cuda.is_available() else (
        dict(), dict(depth=None, ray_b=None), dict(scan=None, known=None, count=None), dict(known=None, count=None),
        dict(cfg=native(range_max=inf, unknown_value=-inf)), dict(cfg=native(alpha=1.0, grid=8)), dict(ra=base, rb=base + 1),
        dict(cs=2, es=1), dict(h=128, w=128, pitch=16384, n=1, mp=base + 4 * 7000, depth=base + 4 * 20000))
    for kw in allowed:
        rc, msg = step(**kw)
        assert rc != 0 and not msg.startswith("rover_elevation_step:"), (kw, rc, msg)
    assert not buf.any()


def test_cfg_classes_check_the_map():
    d = ElevationMapCfg()
    assert (d.cell, d.grid, d.range_min, d.range_max, d.alpha, d.unknown_value) == (0.1, 64, 0.1, 5.0, 1.0, 0.0)
    assert RoverEnvCfg().elevation is None
    d.check()
    c = d.to_native(CameraCfg().position, RayCasterCfg().height_offset)
    assert (c.cell, c.inv_cell, c.grid) == (float(np.float32(0.1)), 10.0, 64) and c.height_offset == float(np.float32(0.26878))
    assert tuple(c.mount_pos) == tuple(float(np.float32(v)) for v in (-0.151, 0.0, 0.73428))
    nan, inf = math.nan, math.inf
    for bad in (dict(grid=4), dict(grid=256), dict(grid=48), dict(grid=0), dict(grid=64.5), dict(cell=0.0), dict(cell=-0.1), dict(cell=nan),
                dict(cell=inf), dict(cell=1e-45), dict(range_min=0.0), dict(range_min=-1.0), dict(range_min=nan), dict(range_min=inf),
                dict(range_min=3.0, range_max=2.0), dict(range_max=nan), dict(alpha=0.0), dict(alpha=1.01), dict(alpha=nan),
                dict(unknown_value=nan)):
        with pytest.raises(ValueError):
            ElevationMapCfg(**bad).check()
    for good in (dict(grid=8), dict(grid=128), dict(range_max=inf), dict(alpha=1e-3), dict(unknown_value=-inf)):
        ElevationMapCfg(**good).check()
    with pytest.raises(ValueError):
        ElevationMapCfg().to_native((0.0, nan, 0.0), 0.25)
    with pytest.raises(ValueError):
        ElevationMapCfg().to_native((0.0, 0.0, 0.0), nan)
    cfg = RoverEnvCfg(elevation=ElevationMapCfg())
    with pytest.raises(ValueError, match="camera"):
        cfg.validate()
    cfg.camera = CameraCfg()
    cfg.validate()
    cfg.camera = CameraCfg(width=129, height=128)
    with pytest.raises(ValueError, match="16384"):
        cfg.validate()
    cfg.camera, cfg.elevation = CameraCfg(), ElevationMapCfg(alpha=2.0)
    with pytest.raises(ValueError, match="alpha"):
        cfg.validate()
    # the classes refuse shapes before any call
    with pytest.raises(ValueError):
        TorchElevationMap(ElevationMapCfg(), CameraCfg(), RayCasterCfg(), 0)
    with pytest.raises(ValueError):
        TorchElevationMap(ElevationMapCfg(), CameraCfg(), RayCasterCfg(), 1, rays=np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError):
        TorchElevationMap(ElevationMapCfg(), CameraCfg(), RayCasterCfg(size=(10.0, 10.0)), 1)     # 101 x 101 rays


def test_body_rays_and_policy_rows():
    import torch
    from camera_reference import ray_dirs_body
    cam = CameraCfg()
    r64 = elevation.body_rays(cam, np.float64)
    assert np.abs(r64 - ray_dirs_body(cam).reshape(-1, 3)).max() <= 1e-15 and np.abs(np.linalg.norm(r64, axis=1) - 1).max() < 1e-15
    r = elevation.body_rays(cam)
    assert r.dtype == np.float32 and r.shape == (14400, 3) and r.flags.c_contiguous and np.array_equal(r, r64.astype(np.float32))
    assert r[:, 0].min() > -0.3 and r[45 * 160 + 80, 0] > 0.5           # the camera looks ahead and down
    rx, ry = elevation.scan_offsets(RayCasterCfg())
    assert rx.shape == ry.shape == (31,) and rx[0] == -1.5 and rx[15] == np.float32(-1.5 + float(np.float32(0.1)) * 15)
    obs, scan = torch.arange(2 * 965, dtype=torch.float32).reshape(2, 965), -torch.ones(2, 961)
    rows = elevation.policy_rows(obs, scan)
    assert torch.equal(rows[:, :4], obs[:, :4]) and torch.equal(rows[:, 4:], scan) and obs[0, 4] == 4.0
    out = torch.empty_like(obs)
    assert elevation.policy_rows(obs, scan, out=out) is out and torch.equal(out, rows)
    with pytest.raises(ValueError):
        elevation.policy_rows(obs, scan[:, :-1])


def test_kernels_use_no_scratch_and_one_map_of_lds():
    """No private segment; a step kernel's LDS is its G x G words of map plus the 8 wave counters (32 bytes), so two workgroups fit
    a CU's 160 KiB even at G = 128; the scan kernel holds the counters only."""
    from helpers import gfx950_code_objects
    from isaac_rover_orbit_amd import build
    build.build_extension()
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("ROCm llvm tools not installed")
    seen = {}
    for blob in gfx950_code_objects(_lib.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True).stdout
        for entry in re.split(r"\n\s*- \.", notes):
            m = re.search(r"\.name:\s*(\S*elevation_(step|scan)_kernel\S*)", entry)
            if not m or ".private_segment_fixed_size" not in entry:
                continue
            G = int(re.search(r"ILi(\d+)E", m.group(1)).group(1)) if m.group(2) == "step" else 0
            assert re.search(r"\.private_segment_fixed_size:\s*0\b", entry), f"{m.group(1)} uses scratch memory"
            lds = int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", entry).group(1))
            assert lds == 4 * G * G + 32 and 2 * lds <= 160 * 1024, (G, lds)
            assert re.search(r"\.max_flat_workgroup_size:\s*512\b", entry)
            assert int(re.search(r"\.vgpr_count:\s*(\d+)", entry).group(1)) <= 128, "four waves per SIMD need <= 128 VGPRs"
            seen[G] = seen.get(G, 0) + 1
    assert seen == {0: 1, 8: 1, 16: 1, 32: 1, 64: 1, 128: 1}


def test_example_flags_make_the_camera_the_sensor_and_the_map():
    import importlib.util
    spec = importlib.util.spec_from_file_location("eval_policy_example", os.path.join(ROOT, "examples", "03_eval_policy.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    ap = ex.build_parser()
    plain = ex.make_cfg(ap.parse_args(["--checkpoint", "x.pt"]))                          # the default: today's loop, no camera
    assert plain.camera is None and plain.elevation is None and plain.scene.num_envs == 1024
    cfg = ex.make_cfg(ap.parse_args(["--checkpoint", "x.pt", "--scan_source", "elevation", "--num_envs", "8"]))
    assert cfg.camera is not None and cfg.camera.sensor is None and cfg.elevation == ElevationMapCfg() and cfg.scene.num_envs == 8
    cfg = ex.make_cfg(ap.parse_args(["--checkpoint", "x.pt", "--scan_source", "elevation", "--depth_range", "0.3", "8", "--depth_sigma",
                                     "0.001", "0", "0.002", "--depth_dropout", "0.01", "0.4", "--map_alpha", "0.5"]))
    s = cfg.camera.sensor
    assert (s.range_min, s.range_max, s.sigma, s.p_drop, s.p_edge, s.invalid_value) == (0.3, 8.0, (0.001, 0.0, 0.002), 0.01, 0.4, 0.0)
    assert cfg.elevation.alpha == 0.5 and cfg.elevation.range_min > s.invalid_value
    cfg.validate()
    one = ex.make_cfg(ap.parse_args(["--checkpoint", "x.pt", "--scan_source", "elevation", "--depth_dropout", "0.1", "0.5"]))
    assert (one.camera.sensor.p_drop, one.camera.sensor.p_edge, one.camera.sensor.range_max) == (0.1, 0.5, math.inf)
    ignored = ex.make_cfg(ap.parse_args(["--checkpoint", "x.pt", "--depth_dropout", "0.1", "0.5"]))   # raycast: the flags do nothing
    assert ignored.camera is None and ignored.elevation is None
