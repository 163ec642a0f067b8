"""The elevation map's min-fill on the CPU (include/rover_elevation_fill.h, isaac_rover_orbit_amd.elevation): TorchElevationMap.fill,
the specification, against a ring-by-ring loop on Python floats; the Chebyshev ball of one cell; the seam of the toroidal
addressing; the lower of two plateaus; a plane seen through the real camera; stability; every refusal of the library (no GPU needed:
the arguments are checked before the device is looked at) and of the cfg class; the default rig; the example's flags; the kernels'
resources from the code object."""
import ctypes as C
import math
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import elevation_cases as cases
from isaac_rover_orbit_amd import _lib
from isaac_rover_orbit_amd.cfg import CameraCfg, ElevationMapCfg, RayCasterCfg, RoverEnvCfg
from isaac_rover_orbit_amd.elevation import TorchElevationMap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS = 0x7FC00000


def f32(x: float) -> float:
    """A Python float rounded to fp32: +, -, *, / and sqrt of fp32 values in double, rounded once more, are fp32 arithmetic."""
    return C.c_float(x).value


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _key(v: float) -> int:
    """The header's key of an fp32 value held in a Python float."""
    b = struct.unpack("<I", struct.pack("<f", v))[0]
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def _cell(v, inv_cell):
    return int(min(max(math.floor(f32(v * inv_cell)), -2 ** 30), 2 ** 30))


def fill_by_hand(h, iterations):
    """The window `h` (G x G nested lists of Python floats, NaN = unknown; changed in place) through the header's step 2 as a
    breadth-first search by Chebyshev rings: ring k is collected in full before any of it is written.  Returns dist."""
    G = len(h)
    dist = [[255 if math.isnan(v) else 0 for v in row] for row in h]
    for k in range(1, iterations + 1):
        ring = []
        for i in range(G):
            for j in range(G):
                if dist[i][j] != 255:
                    continue
                near = [h[i + di][j + dj] for di in (-1, 0, 1) for dj in (-1, 0, 1)
                        if (di or dj) and 0 <= i + di < G and 0 <= j + dj < G and dist[i + di][j + dj] < k]
                if near:
                    ring.append((i, j, min(near, key=_key)))
        if not ring:
            break
        for i, j, v in ring:
            h[i][j], dist[i][j] = v, k
    return dist


def scan_by_hand(c, ray_x, ray_y, h, dist, origin, pos, quat):
    """Step 4 on Python floats over the filled window `h` / `dist` (window order).  Returns (scan, dist per column)."""
    G = c.grid
    n_cols = len(ray_x) * len(ray_y)
    if not all(math.isfinite(v) for v in (*pos, *quat)):
        return [c.unknown_value] * n_cols, [255] * n_cols
    px, py, pz = pos
    w, x, y, z = quat
    lo = (origin[0] - G // 2, origin[1] - G // 2)
    a = f32(1 - f32(2 * f32(f32(y * y) + f32(z * z))))
    b = f32(2 * f32(f32(w * z) + f32(x * y)))
    inv = f32(1 / f32(math.sqrt(f32(f32(a * a) + f32(b * b)))))
    cyaw, syaw = f32(a * inv), f32(b * inv)
    scan, col_dist = [], []
    for oy in ray_y:
        for ox in ray_x:
            sx_ = f32(px + f32(f32(cyaw * ox) - f32(syaw * oy)))
            sy_ = f32(py + f32(f32(syaw * ox) + f32(cyaw * oy)))
            gx, gy = _cell(sx_, c.inv_cell), _cell(sy_, c.inv_cell)
            d = dist[gy - lo[1]][gx - lo[0]] if (lo[0] <= gx < lo[0] + G and lo[1] <= gy < lo[1] + G) else 255
            col_dist.append(d)
            scan.append(c.unknown_value if d == 255 else f32(f32(pz - h[gy - lo[1]][gx - lo[0]]) - c.height_offset))
    return scan, col_dist


def _spec(G, n=1, cell=0.25, **kw):
    ecfg, cam, sc = cases.cfgs(12, 16, G, cell=cell, **kw)
    return TorchElevationMap(ecfg, cam, sc, n)


def _put_window(spec, e, window, origin):
    """Writes the window (G x G, window order) of env `e` into the spec's slot-addressed map, by a loop of its own."""
    G = spec.grid
    spec.origin[e] = origin
    lo = (origin[0] - G // 2, origin[1] - G // 2)
    for i in range(G):
        for j in range(G):
            spec.map[e, (lo[1] + i) % G, (lo[0] + j) % G] = window[i][j]


def _window_of(spec, e, arr):
    G = spec.grid
    lo = (int(spec.origin[e, 0]) - G // 2, int(spec.origin[e, 1]) - G // 2)
    return np.array([[arr[e, (lo[1] + i) % G, (lo[0] + j) % G] for j in range(G)] for i in range(G)])


SPECIAL = [-0.0, 0.0, 1e-42, -1e-42, 3e38, -3e38, -1.25, 0.5]      # +-0, denormals, near the fp32 maximum, both signs


def random_window(rng, G, known):
    """G x G Python floats (fp32 values): `known` is a share, or "one" for a single known cell; the known heights are normal draws
    with the SPECIAL values strewn in."""
    h = rng.standard_normal((G, G)).astype(np.float32)
    sp = rng.random((G, G)) < 0.3
    h[sp] = np.array(SPECIAL, np.float32)[rng.integers(0, len(SPECIAL), sp.sum())]
    if known == "one":
        mask = np.zeros((G, G), bool)
        mask[rng.integers(G), rng.integers(G)] = True
    else:
        mask = rng.random((G, G)) < known
    h[~mask] = np.nan
    return [[float(v) for v in row] for row in h]


@pytest.mark.parametrize("known", [0.0, "one", 0.05, 0.5, 1.0])
@pytest.mark.parametrize("G", [8, 16])
def test_spec_against_a_hand_written_ring_loop(G, known):
    """Three envs with different windows and origins (negative, lo no multiple of G) and three sweep counts; filled, cell dist, scan,
    column dist and count against the loops above, bit for bit.  With cell = 0.25 the 3 m scan leaves the 2 m window at G = 8."""
    n = 3
    spec = _spec(G, n, unknown_value=-7.5)
    c = spec.cfg
    rx, ry = [float(v) for v in spec.ray_x], [float(v) for v in spec.ray_y]
    rng = np.random.default_rng(100 * G + (7 if known == "one" else int(known * 20)))
    origins = [(-3, 5), (G + 1, -2 * G - 3), (0, 0)]
    windows = [random_window(rng, G, known) for _ in range(n)]
    for e in range(n):
        _put_window(spec, e, windows[e], origins[e])
    pos = np.array([[(o[0] + 0.3) * 0.25, (o[1] + 0.6) * 0.25, 0.3 + 0.1 * e] for e, o in enumerate(origins)], np.float32)
    quat = np.stack([cases.quat(0.4 + 1.9 * e, 0.03, -0.02) for e in range(n)])
    before = spec.map.copy(), spec.origin.copy()
    seen = set()
    for iterations in (1, 3, 254):
        scan, col_dist, count, filled, cell_dist = spec.fill(pos, quat, iterations=iterations)
        assert scan.dtype == filled.dtype == np.float32 and col_dist.dtype == cell_dist.dtype == np.uint8 and count.dtype == np.int32
        for e in range(n):
            h = [row[:] for row in windows[e]]
            dist = fill_by_hand(h, iterations)
            assert np.array_equal(_bits(_window_of(spec, e, filled).astype(np.float32)), _bits(np.array(h, np.float32))), (iterations, e)
            assert _window_of(spec, e, cell_dist).tolist() == dist, (iterations, e)
            hs, hd = scan_by_hand(c, rx, ry, h, dist, origins[e], [float(v) for v in pos[e]], [float(v) for v in quat[e]])
            assert np.array_equal(_bits(scan[e]), _bits(np.array(hs, np.float32))) and col_dist[e].tolist() == hd, (iterations, e)
            assert count[e] == sum(d < 255 for d in hd)
            seen |= set(hd)
    assert np.array_equal(_bits(spec.map), _bits(before[0])) and np.array_equal(spec.origin, before[1])      # read only
    if known in (0.0,):
        assert seen == {255}
    elif known == 1.0:
        assert 0 in seen and seen <= {0, 255}                                # 255: the columns outside the window
    else:                                                                    # the inputs do exercise several rings
        assert 0 in seen and 1 in seen and (known == 0.5 or max(seen - {255}) >= 3)


@pytest.mark.parametrize("G", [8, 16])
def test_one_cell_fills_its_chebyshev_ball(G):
    """One known cell in the centre: after k sweeps exactly the cells within Chebyshev distance k hold its value, and dist is that
    distance.  A sweep that read its own writes (Gauss-Seidel, in place) would fill the whole lower right quadrant in sweep 1."""
    spec = _spec(G)
    ci = cj = G // 2
    window = [[math.nan] * G for _ in range(G)]
    window[ci][cj] = -0.75
    _put_window(spec, 0, window, (5, -9))
    cheb = np.maximum(np.abs(np.arange(G)[:, None] - ci), np.abs(np.arange(G)[None, :] - cj))
    for k in (1, 2, 3, G // 2 - 1, G // 2, 254):
        filled, dist = spec.fill_window(k)
        f, d = _window_of(spec, 0, filled), _window_of(spec, 0, dist)
        inside = cheb <= k
        assert np.array_equal(d, np.where(inside, cheb, 255)), k
        assert (f[inside] == -0.75).all() and np.isnan(f[~inside]).all(), k


def test_the_seam_is_no_neighbourhood():
    """One known cell at window (3, 0) of a window whose low corner (-11, -3) is negative and no multiple of G: one sweep fills its
    five neighbours inside the window; (3, G - 1), the adjacent SLOT across the seam, stays unknown, as do rows 2 - 4 of column
    G - 1 altogether."""
    G = 16
    spec = _spec(G)
    window = [[math.nan] * G for _ in range(G)]
    window[3][0] = 2.5
    _put_window(spec, 0, window, (-3, 5))
    assert tuple(spec.origin[0] - G // 2) == (-11, -3)
    filled, dist = spec.fill_window(1)
    d = _window_of(spec, 0, dist)
    want = np.full((G, G), 255)
    want[2:5, 0:2] = 1
    want[3, 0] = 0
    assert np.array_equal(d, want) and (d < 255).sum() == 6 and d[3, G - 1] == 255
    f = _window_of(spec, 0, filled)
    assert (f[d < 255] == 2.5).all() and np.isnan(f[d == 255]).all()


def test_the_lower_of_two_plateaus_wins_and_minus_zero_beats_zero():
    """Columns 0 - 2 at 1.0, columns 4 - 7 at -2.0: column 3 touches both and takes -2.0.  With +0 and -0 it takes -0 (the order of
    the keys; a float comparison calls them equal).  Both also with the plateaus swapped."""
    G = 8
    spec = _spec(G)
    for left, right, want in ((1.0, -2.0, -2.0), (-2.0, 1.0, -2.0), (0.0, -0.0, -0.0), (-0.0, 0.0, -0.0)):
        window = [[left] * 3 + [math.nan] + [right] * 4 for _ in range(G)]
        _put_window(spec, 0, window, (2, 3))
        filled, dist = spec.fill_window(5)
        f, d = _window_of(spec, 0, filled).astype(np.float32), _window_of(spec, 0, dist)
        assert (d[:, 3] == 1).all() and (np.delete(d, 3, 1) == 0).all()
        assert (_bits(f[:, 3]) == _bits(np.float32(want))).all(), (left, right)


_PLANE_POSES = [(z, yaw) for z in (0.2, 0.3, 0.4, 0.5) for yaw in (0.0, 0.3, 0.785)]


@pytest.fixture(scope="module")
def plane_map():
    """tests/test_elevation.py::plane_frames built again: a terrain at height c through the default camera at its twelve poses (the
    camera's float64 reference), and the default map after ONE frame of each."""
    from camera_reference import render
    c, cam, sc = 0.37, CameraCfg(), RayCasterCfg()
    pos = np.array([[51.23 + 0.7 * k, 48.91 - 0.4 * k, c + z] for k, (z, _) in enumerate(_PLANE_POSES)])
    quat = np.stack([[math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)] for _, yaw in _PLANE_POSES])
    depth, _ = render(cam, np.full((1024, 1024), c), 0.1, 0.0, 0.0, pos, quat)
    spec = TorchElevationMap(ElevationMapCfg(), cam, sc, len(pos))
    p, q = pos.astype(np.float32), quat.astype(np.float32)
    raw = spec.update(depth.reshape(len(pos), -1).astype(np.float32), p, q)
    return c, sc, spec, p, q, raw


def test_a_plane_through_the_real_camera_fills_in_sixteen_sweeps(plane_map):
    """One frame knows about half of the 961 columns.  16 sweeps fill all 961 at all twelve poses, 12 sweeps do not; every filled
    column reads pos.z - c - height_offset within 8 ulp of 5 m, the bound of the raw scan's own test: a minimum of measured cells is
    one of them.  The measured columns keep the raw scan's bits."""
    c, sc, spec, p, q, (raw_scan, raw_known, raw_count) = plane_map
    scan, dist, count, _, _ = spec.fill(p, q, iterations=16)
    print(f"measured {raw_count.min()} .. {raw_count.max()}, after 16 sweeps {count.min()} .. {count.max()}")
    assert (count == 961).all() and (dist < 255).all() and dist.max() <= 16
    assert np.array_equal(dist == 0, raw_known.astype(bool)) and np.array_equal(_bits(scan)[dist == 0], _bits(raw_scan)[dist == 0])
    want = (p[:, 2].astype(np.float64) - c - sc.height_offset)[:, None]
    err = np.abs(scan.astype(np.float64) - want).max()
    print(f"largest error of a filled column {err:.3e} m")
    assert err <= 8 * float(np.spacing(np.float32(5.0)))
    scan12, dist12, count12, _, _ = spec.fill(p, q, iterations=12)
    print(f"after 12 sweeps {count12.min()} .. {count12.max()}")
    assert count12.min() < 961 and (count12 >= raw_count).all() and np.array_equal(count12, (dist12 < 255).sum(1))
    k = dist12 < 255
    assert np.array_equal(_bits(scan12)[k], _bits(scan)[k]) and np.array_equal(dist12[k], dist[k]) and (scan12[~k] == 0.0).all()
    assert np.abs(scan12.astype(np.float64) - want)[k].max() <= 8 * float(np.spacing(np.float32(5.0)))


def test_more_sweeps_than_needed_known_maps_and_empty_maps(plane_map):
    """More iterations than the fill needs give the same bits; a fully known map comes back as it is, its scan the raw scan, dist
    all 0; an all-unknown map stays unknown with count 0."""
    _, _, plane, p, q, _ = plane_map
    a, b = plane.fill(p, q, iterations=64), plane.fill(p, q, iterations=254)
    assert a[3].shape == plane.map.shape and not np.isnan(a[3]).any()            # 64 >= G - 1: the whole window
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    G, n = 16, 2
    spec = _spec(G, n)
    rng = np.random.default_rng(4)
    spec.map[...] = rng.standard_normal((n, G, G)).astype(np.float32)
    spec.map[0, 3, 4], spec.map[1, 0, 0], spec.map[1, 15, 15] = -0.0, np.inf, -np.inf      # only a NaN is unknown
    spec.origin[...] = [[-3, 5], [17, -40]]
    pos = np.array([[-0.7, 1.3, 0.3], [4.3, -9.9, 0.5]], np.float32)
    quat = np.stack([cases.quat(0.4), cases.quat(-2.0)])
    raw = spec.scan(pos, quat)
    scan, dist, count, filled, cell_dist = spec.fill(pos, quat, iterations=7)
    assert np.array_equal(_bits(filled), _bits(spec.map)) and not cell_dist.any()
    assert np.array_equal(_bits(scan), _bits(raw[0])) and np.array_equal(count, raw[2]) and (count > 900).all()
    assert np.array_equal(dist, np.where(raw[1] == 1, 0, 255))                 # 255: the few columns outside the window
    spec.clear()
    scan, dist, count, filled, cell_dist = spec.fill(pos, quat, iterations=254)
    assert np.isnan(filled).all() and (cell_dist == 255).all() and (dist == 255).all() and not count.any()
    assert (scan == spec.cfg.unknown_value).all()
    assert np.array_equal(_bits(filled), _bits(spec.map))
    # a bad pose: the row is unknown, the window outputs are what they are for any pose
    spec.map[0, 2, 2] = 1.0
    bad = pos.copy()
    bad[0, 1] = np.nan
    scan, dist, count, filled, cell_dist = spec.fill(bad, quat, iterations=3)
    assert (dist[0] == 255).all() and count[0] == 0 and (scan[0] == spec.cfg.unknown_value).all() and (cell_dist[0] < 255).sum() > 9
    with pytest.raises(ValueError):
        spec.fill(pos, quat, iterations=0)
    with pytest.raises(ValueError):
        spec.fill(pos, quat, iterations=255)
    with pytest.raises(ValueError):
        TorchElevationMap(ElevationMapCfg(), CameraCfg(), RayCasterCfg(), 1, float64=True).fill_window(3)


def test_every_refusal_through_the_library():
    lib = _lib.load()
    assert lib.rover_elevation_fill_cfg_bytes() == C.sizeof(_lib.ElevationFillCfg) == 4
    buf = np.zeros(8192, np.float32)
    base = buf.ctypes.data                               # never read or written: every call below is refused
    nan, inf = math.nan, math.inf
    MAP, ORG, POSE, RX, RY, SCAN, SDIST, COUNT, FILLED, CDIST = (base + 4 * o for o in (0, 512, 2816, 2880, 2912, 3072, 4096, 4160, 4608, 5632))

    def native(**kw):
        c = ElevationMapCfg(grid=16, cell=0.25).to_native((0.1, 0.0, 0.7), 0.25)
        for k, v in kw.items():
            if k == "mount_pos":
                for i in range(3):
                    c.mount_pos[i] = v[i]
            else:
                setattr(c, k, v)
        return c

    def fill(cfg=None, null_cfg=False, it=5, null_fill=False, pos=POSE, quat=POSE + 12, cs=1, es=7, mp=MAP, org=ORG, rx=RX, nx=5, ry=RY,
             ny=4, scan=SCAN, sp=20, sdist=SDIST, count=COUNT, filled=FILLED, cdist=CDIST, n=2):
        cfg = cfg if cfg is not None else native()
        fc = _lib.ElevationFillCfg(it)
        rc = lib.rover_elevation_fill(None if null_cfg else C.byref(cfg), None if null_fill else C.byref(fc), pos, quat, cs, es, mp, org,
                                      rx, nx, ry, ny, scan, sp, sdist, count, filled, cdist, n, None)
        return rc, lib.rover_last_error().decode()

    invalid = [
        (dict(null_cfg=True), "NULL"), (dict(null_fill=True), "NULL"), (dict(pos=None), "NULL"), (dict(quat=None), "NULL"),
        (dict(mp=None), "NULL"), (dict(org=None), "NULL"), (dict(rx=None), "NULL"), (dict(ry=None), "NULL"),
        (dict(scan=None, filled=None), "NULL"), (dict(scan=None, filled=None, rx=None, ry=None), "NULL"),
        (dict(scan=None, mp=None), "NULL"),
        (dict(it=0), "iterations"), (dict(it=-1), "iterations"), (dict(it=255), "iterations"), (dict(it=2 ** 31 - 1), "iterations"),
        (dict(n=0), "n must"), (dict(n=-3), "n must"), (dict(nx=0), "nx and ny"), (dict(ny=-1), "nx and ny"),
        (dict(scan=None, nx=0), "nx and ny"), (dict(cs=0), "stride"), (dict(es=-7), "stride"),
        (dict(pos=POSE + 2), "aligned"), (dict(quat=POSE + 13), "aligned"), (dict(mp=MAP + 1), "aligned"), (dict(org=ORG + 2), "aligned"),
        (dict(rx=RX + 3), "aligned"), (dict(ry=RY + 1), "aligned"), (dict(scan=SCAN + 2), "aligned"), (dict(count=COUNT + 1), "aligned"),
        (dict(filled=FILLED + 2), "aligned"),
        (dict(sp=19), "scan_pitch"),
        (dict(cfg=native(cell=0.0)), "cell"), (dict(cfg=native(cell=inf)), "cell"), (dict(cfg=native(cell=nan)), "cell"),
        (dict(cfg=native(inv_cell=-4.0)), "cell"), (dict(cfg=native(inv_cell=nan)), "cell"), (dict(cfg=native(inv_cell=inf)), "cell"),
        (dict(cfg=native(range_min=0.0)), "range_min"), (dict(cfg=native(range_min=-0.1)), "range_min"),
        (dict(cfg=native(range_min=nan)), "range_min"), (dict(cfg=native(range_min=inf)), "range_min"),
        (dict(cfg=native(range_min=2.0, range_max=1.0)), "range_max"), (dict(cfg=native(range_max=nan)), "range_max"),
        (dict(cfg=native(alpha=0.0)), "alpha"), (dict(cfg=native(alpha=1.5)), "alpha"), (dict(cfg=native(alpha=nan)), "alpha"),
        (dict(cfg=native(unknown_value=nan)), "unknown_value"), (dict(cfg=native(height_offset=nan)), "height_offset"),
        (dict(cfg=native(mount_pos=(0.0, inf, 0.0))), "mount_pos"), (dict(cfg=native(mount_pos=(nan, 0.0, 0.0))), "mount_pos"),
        (dict(scan=MAP + 4 * 100), "overlap"), (dict(mp=SCAN + 4 * 39), "overlap"), (dict(mp=SCAN - 4 * 511), "overlap"),
        (dict(filled=MAP + 4 * 511), "overlap"), (dict(filled=MAP - 4 * 511), "overlap"), (dict(filled=MAP), "overlap"),
        (dict(filled=SCAN + 4 * 39), "overlap"), (dict(filled=SCAN - 4 * 511), "overlap"), (dict(scan=FILLED + 4 * 8), "overlap"),
    ]
    for kw, text in invalid:
        rc, msg = fill(**kw)
        assert rc == 1 and msg.startswith("rover_elevation_fill:") and text in msg, (kw, rc, msg)
    for kw, text in ((dict(cfg=native(grid=4)), "power of two"), (dict(cfg=native(grid=256)), "power of two"),
                     (dict(cfg=native(grid=24)), "power of two"), (dict(cfg=native(grid=0)), "power of two"),
                     (dict(nx=65, ny=64, sp=65 * 64), "4096"), (dict(scan=None, nx=65, ny=64), "4096")):
        rc, msg = fill(**kw)
        assert rc == 4 and msg.startswith("rover_elevation_fill:") and text in msg, (kw, rc, msg)
    assert not buf.any()
    # on a host without a GPU, what is allowed gets past the argument checks and fails at the device query, with nothing written
    allowed = () if torch.cuda.is_available() else (
        dict(), dict(it=1), dict(it=254), dict(filled=None, cdist=None), dict(sdist=None, count=None), dict(scan=None, rx=None, ry=None),
        dict(scan=None, sdist=None, count=None, cdist=None), dict(cfg=native(range_max=inf, unknown_value=-inf, grid=8)),
        dict(cs=2, es=1), dict(filled=MAP + 4 * 512), dict(filled=SCAN + 4 * 40))
    for kw in allowed:
        rc, msg = fill(**kw)
        assert rc != 0 and not msg.startswith("rover_elevation_fill:"), (kw, rc, msg)
    assert not buf.any()


def test_the_cfg_class_checks_the_fill():
    d = ElevationMapCfg()
    assert (d.fill, d.fill_iterations) == ("none", 32) and ElevationMapCfg() == ElevationMapCfg()
    d.check()
    for bad in (dict(fill="max"), dict(fill=None), dict(fill=""), dict(fill="MIN"), dict(fill_iterations=0), dict(fill_iterations=-1),
                dict(fill_iterations=255), dict(fill_iterations=3.5), dict(fill_iterations=math.nan), dict(fill_iterations="8"),
                dict(fill_iterations=True), dict(fill="min", fill_iterations=1000)):
        with pytest.raises(ValueError):
            ElevationMapCfg(**bad).check()
    for good in (dict(fill="min"), dict(fill="min", fill_iterations=1), dict(fill="min", fill_iterations=254), dict(fill_iterations=64)):
        ElevationMapCfg(**good).check()
    cfg = RoverEnvCfg(camera=CameraCfg(), elevation=ElevationMapCfg(fill="min", fill_iterations=300))
    with pytest.raises(ValueError, match="fill_iterations"):
        cfg.validate()
    cfg.elevation.fill_iterations = 20
    cfg.validate()
    # the native struct of the map is what it was: the fill's parameters travel in a struct of their own
    c = ElevationMapCfg(fill="min").to_native(CameraCfg().position, 0.25)
    assert C.sizeof(c) == 44 and bytes(c) == bytes(ElevationMapCfg().to_native(CameraCfg().position, 0.25))


def test_the_rig_fills_behind_every_map_launch_and_not_by_default():
    """On the CPU over test_sensor_rig's stand-ins.  Default: no key, no buffers, no stage.  With fill_iterations = 5: one fill
    behind every map launch (reset, steps, a reset with draws), with the map launch's pose, into rotating buffers published under
    the three new keys; the three old keys hold what the map launch wrote."""
    import test_sensor_rig as rig_cases
    from isaac_rover_orbit_amd.envs._sensors import FILL_KEYS, KEYS, SensorRig
    assert FILL_KEYS == ("elevation_scan_filled", "elevation_fill_dist", "elevation_filled_count") and not set(FILL_KEYS) & set(KEYS)
    for source in ("camera", "lidar"):
        host, log, rig, _ = rig_cases.build(True, True, source)
        rig.update(force=True)
        assert rig.fill_iterations == 0 and not hasattr(rig, "_fills") and not set(FILL_KEYS) & set(host.extras)
        assert [name for name, _ in log].count("map") == 1

    class FillingMap(rig_cases.MapStandIn):
        def fill(self, pos, quat, scan_out=None, dist_out=None, count_out=None, iterations=None):
            scan_out.fill_(500 + self.calls), dist_out.fill_(self.calls), count_out.fill_(10 + self.calls)
            self.log.append(("fill", {"pos": pos, "quat": quat, "outs": (scan_out, dist_out, count_out), "iterations": iterations}))

    N, COLS = rig_cases.N, rig_cases.COLS
    for source, camera in (("camera", True), ("lidar", False)):
        host, log = rig_cases.Host(), []
        host.extras["elevation_scan_filled"] = "stale"
        pose = (torch.zeros(N, 3), torch.zeros(N, 4))
        kw = dict(pose=pose, elevation=FillingMap(log), map_source=source, unknown_value=-1.0, fill_iterations=5)
        if camera:
            kw.update(render=lambda cfg, ws, buf: buf.fill_(1.0), camera_cfg="camera-cfg", workspace="workspace", image=(rig_cases.H, rig_cases.W))
        else:
            kw.update(lidar=rig_cases.LidarStandIn(log))
        rig = SensorRig(host, "cpu", N, **kw)
        ex = host.extras
        assert ex["elevation_scan_filled"].shape == (N, COLS) and bool((ex["elevation_scan_filled"] == -1.0).all())
        assert ex["elevation_fill_dist"].dtype == torch.uint8 and bool((ex["elevation_fill_dist"] == 255).all())
        assert ex["elevation_filled_count"].dtype == torch.int32 and ex["elevation_filled_count"].shape == (N,)
        previous = None
        for call, kind in enumerate(["reset", "step", "step", "draws", "step"], 1):
            del log[:]
            host.call_counter += 1
            if kind == "reset":
                rig.clear()
                rig.update(force=True)
            elif kind == "draws":
                rig.update_after_draws(torch.tensor([0, 1, 0], dtype=torch.uint8))
            else:
                host.common_step_counter += 1
                rig.update()
            names = [name for name, _ in log if name in ("map", "fill")]
            assert names == ["map", "fill"], (kind, names)
            m, f = dict(log)["map"], dict(log)["fill"]
            assert f["pos"] is m["pos"] is pose[0] and f["quat"] is pose[1] and f["iterations"] == 5
            assert all(o is ex[k] for o, k in zip(f["outs"], FILL_KEYS)) and all(o is ex[k] for o, k in zip(m["outs"], KEYS[5:]))
            assert bool((ex["elevation_scan_filled"] == 500 + call).all()) and bool((ex["elevation_scan"] == 300 + call).all())
            assert bool((ex["elevation_filled_count"] == 10 + call).all()) and bool((ex["elevation_fill_dist"] == call).all())
            if previous is not None:                                         # the frame before this one was not written over
                assert all(o is not p for o, p in zip(f["outs"], previous[0])) and bool((previous[0][0] == previous[1]).all())
            previous = (f["outs"], 500 + call)
        assert set(rig.state_dict()) == {"elevation_map", "elevation_origin"}


def test_example_flags_switch_the_fill_on():
    import importlib.util
    spec = importlib.util.spec_from_file_location("eval_policy_example_fill", os.path.join(ROOT, "examples", "03_eval_policy.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    ap = ex.build_parser()
    plain = ex.make_cfg(ap.parse_args(["--checkpoint", "x.pt"]))
    assert plain.elevation is None and plain.camera is None
    cfg = ex.make_cfg(ap.parse_args(["--checkpoint", "x.pt", "--scan_source", "elevation"]))
    assert cfg.elevation.fill == "none" and cfg.elevation == ElevationMapCfg()
    for extra, source in (([], "camera"), (["--map_source", "lidar"], "lidar")):
        cfg = ex.make_cfg(ap.parse_args(["--checkpoint", "x.pt", "--scan_source", "elevation", "--map_fill", "min", "--map_fill_iterations",
                                         "20", *extra]))
        assert (cfg.elevation.fill, cfg.elevation.fill_iterations, cfg.elevation.source) == ("min", 20, source)
        cfg.validate()
    with pytest.raises(SystemExit):
        ap.parse_args(["--checkpoint", "x.pt", "--map_fill", "mean"])
    bad = ex.make_cfg(ap.parse_args(["--checkpoint", "x.pt", "--scan_source", "elevation", "--map_fill", "min", "--map_fill_iterations", "0"]))
    with pytest.raises(ValueError, match="fill_iterations"):
        bad.validate()


def test_fill_kernels_use_no_scratch_and_bounded_lds():
    """Each of the five instantiations: no private segment, static LDS <= 9 G^2 + 256 bytes (the float image, the byte image, two
    bit images and the counters are 5 G^2 + G^2 / 4 + 40 from G = 32 on), 512 threads."""
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
            m = re.search(r"\.name:\s*(\S*elevation_fill_kernel\S*)", entry)
            if not m or ".private_segment_fixed_size" not in entry:
                continue
            assert "elevation_step_kernel" not in m.group(1) and "elevation_scan_kernel" not in m.group(1)
            G = int(re.search(r"ILi(\d+)E", m.group(1)).group(1))
            assert re.search(r"\.private_segment_fixed_size:\s*0\b", entry), f"{m.group(1)} uses scratch memory"
            lds = int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", entry).group(1))
            assert lds <= 9 * G * G + 256 and lds <= 160 * 1024, (G, lds)
            assert re.search(r"\.max_flat_workgroup_size:\s*512\b", entry)
            seen[G] = seen.get(G, 0) + 1
    assert seen == {8: 1, 16: 1, 32: 1, 64: 1, 128: 1}
