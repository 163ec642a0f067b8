"""The elevation map's min-fill as one HIP launch on the MI355X (include/rover_elevation_fill.h) against TorchElevationMap.fill, its
CPU specification.

Everything here is BIT-EQUAL on the five outputs (scan, column dist, count, filled window, cell dist): the kernel is comparisons,
integer cell arithmetic, an integer minimum of key bits and the scan's correctly rounded fp32 operations in a fixed order, and
numpy does the same, so equality is derived, not measured.  Every launch must leave `map` and `origin` as they were.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import elevation_cases as cases
from isaac_rover_orbit_amd import _fused, _lib
from isaac_rover_orbit_amd.cfg import RayCasterCfg

pytestmark = pytest.mark.gpu

GAP_BITS = 0x7FC0BEEF                                  # a NaN with a payload: what the frames around the buffers hold
NAMES = ("scan", "column dist", "count", "filled", "cell dist")
SPECIAL = np.array([-0.0, 0.0, 1e-42, -1e-42, 3e38, -3e38, np.inf, -np.inf], np.float32)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _pair(n, G, cell=None, scanner=None, **kw):
    from isaac_rover_orbit_amd.elevation import ElevationMap, TorchElevationMap
    ecfg, cam, sc = cases.cfgs(12, 16, G, cell=cell or (0.25 if G <= 16 else 0.1), **kw)
    sc = scanner or sc
    return ElevationMap(ecfg, cam, sc, n, "cuda"), TorchElevationMap(ecfg, cam, sc, n)


def _origins(n, G):
    """Negative coordinates, and a low corner that is no multiple of G on either axis."""
    o = np.array([(-3, 5), (G + 1, -2 * G - 3), (-G // 2 + 5, G // 2 - 7), (7, -1)][:n], np.int32)
    assert (((o - G // 2) & (G - 1)) != 0).all() and (o < 0).any()
    return o


def _random_maps(rng, n, G, known):
    m = rng.standard_normal((n, G, G)).astype(np.float32)
    sp = rng.random((n, G, G)) < 0.2
    m[sp] = SPECIAL[rng.integers(0, len(SPECIAL), sp.sum())]
    m[rng.random((n, G, G)) >= known] = np.nan
    return m


def _load(dev, spec, maps, origins):
    spec.map[...] = maps
    spec.origin[...] = origins
    dev.map.copy_(torch.from_numpy(spec.map))
    dev.origin.copy_(torch.from_numpy(spec.origin))


def _near(spec, shift=(0.3, 0.6), z=0.3):
    """Poses in the centre cell of each env's window, the yaw in another quadrant per env."""
    n, cell = spec.num_envs, float(spec.map_cfg.cell)
    pos = np.array([[(o[0] + shift[0]) * cell, (o[1] + shift[1]) * cell, z + 0.1 * e] for e, o in enumerate(spec.origin)], np.float32)
    return pos, np.stack([cases.quat(0.4 + 1.9 * e, 0.03, -0.02) for e in range(n)])


def _poses(pos, quat, layout):
    both = torch.from_numpy(np.concatenate([pos, quat], 1).astype(np.float32)).cuda()
    if layout == "soa":
        st = both.t().contiguous()                     # (7, n): the env's state rows
        return st[0:3].t(), st[3:7].t()
    return both[:, :3], both[:, 3:]


def _check(dev, spec, pos, quat, iterations, layout="aos", what="", **outs):
    m0, o0 = dev.map.clone(), dev.origin.clone()
    got = dev.fill(*_poses(pos, quat, layout), iterations=iterations, filled_out=True, cell_dist_out=True, **outs)
    want = spec.fill(pos, quat, iterations=iterations)
    torch.cuda.synchronize()
    for g, w, nm in zip(got, want, NAMES):
        assert np.array_equal(_bits(g).reshape(w.shape), _bits(w)), f"{what}: {nm}"
    assert torch.equal(dev.map.view(torch.int32), m0.view(torch.int32)) and torch.equal(dev.origin, o0), f"{what}: map or origin written"
    return got, want


@pytest.mark.parametrize("G", [8, 16, 64, 128])
def test_random_maps_at_every_kind_of_grid(G):
    """n = 3, 5 % and 50 % known, heights with +-0, denormals, +-3e38 and +-inf; G = 8 has fewer cells than threads, 64 and 128
    8 and 32 cells per thread.  Every measured slot of the filled window is the map's own bits."""
    n = 3
    dev, spec = _pair(n, G, unknown_value=-7.5)
    rng = np.random.default_rng(G)
    for known in (0.05, 0.5):
        _load(dev, spec, _random_maps(rng, n, G, known), _origins(n, G))
        pos, quat = _near(spec)
        for iterations in (3, 254):
            got, want = _check(dev, spec, pos, quat, iterations, what=f"{known} known, {iterations} sweeps")
            measured = ~np.isnan(spec.map)
            assert np.array_equal(_bits(got[3])[measured], _bits(spec.map)[measured]) and measured.any() and not measured.all()
            assert (want[4] == 0).sum() == measured.sum() and want[2].max() > 0


@pytest.mark.parametrize("iterations", [1, 2, 31, 254])
def test_sweep_counts(iterations):
    """G = 64 with about 1 cell in 300 known, so that 31 sweeps still fill something and the early exit comes before 254."""
    n, G = 3, 64
    dev, spec = _pair(n, G)
    _load(dev, spec, _random_maps(np.random.default_rng(9), n, G, 0.003), _origins(n, G))
    pos, quat = _near(spec)
    _, want = _check(dev, spec, pos, quat, iterations)
    reach = int(want[4][want[4] < 255].max())
    assert reach == min(iterations, reach) and (iterations > 2 or reach == iterations) and (iterations < 31 or reach > 2)
    assert iterations != 254 or (reach < 254 and (want[4] < 255).all())


@pytest.mark.parametrize("layout", ["soa", "aos"])
def test_seam_and_centre_cell_in_both_pose_layouts(layout):
    """Env 0: one known cell at window (3, 0), low corner (-11, -3): one sweep fills its five in-window neighbours and leaves
    (3, G - 1), the adjacent slot, unknown.  Env 1: one cell in the centre, k sweeps fill its Chebyshev ball exactly."""
    n, G = 2, 16
    dev, spec = _pair(n, G)
    maps = np.full((n, G, G), np.nan, np.float32)
    origins = np.array([(-3, 5), (21, -40)], np.int32)
    lo = origins - G // 2
    maps[0, (lo[0, 1] + 3) % G, (lo[0, 0] + 0) % G] = 2.5
    maps[1, (lo[1, 1] + G // 2) % G, (lo[1, 0] + G // 2) % G] = -0.75
    _load(dev, spec, maps, origins)
    pos, quat = _near(spec)
    for k in (1, 2, 5, 254):
        got, _ = _check(dev, spec, pos, quat, k, layout=layout, what=f"{k} sweeps")
        dist = got[4].cpu().numpy()
        window = lambda e: np.array([[dist[e, (lo[e, 1] + i) % G, (lo[e, 0] + j) % G] for j in range(G)] for i in range(G)])   # noqa: E731
        cheb = np.maximum(np.abs(np.arange(G)[:, None] - G // 2), np.abs(np.arange(G)[None, :] - G // 2))
        assert np.array_equal(window(1), np.where(cheb <= k, cheb, 255))
        if k == 1:
            w0 = window(0)
            assert (w0 < 255).sum() == 6 and w0[3, 0] == 0 and (w0[2:5, 0:2] < 255).all() and (w0[:, G - 1] == 255).all()


@pytest.mark.parametrize("word", range(7))
def test_a_bad_pose_word_gives_an_unknown_row_and_a_written_window(word):
    """NaN (env 1) and inf (env 2) in each of the seven pose floats in turn: dist 255, count 0, the row unknown_value; the filled
    window and its dist are written all the same, and env 0 is served as usual."""
    n, G = 3, 16
    dev, spec = _pair(n, G, unknown_value=-7.5)
    _load(dev, spec, _random_maps(np.random.default_rng(3), n, G, 0.3), _origins(n, G))
    pos, quat = _near(spec)
    pose = np.concatenate([pos, quat], 1)
    pose[1, word], pose[2, word] = np.nan, -np.inf if word % 2 else np.inf
    for layout in ("aos", "soa"):
        filled = torch.full((n, G, G), GAP_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
        got, want = _check(dev, spec, pose[:, :3], pose[:, 3:], 4, layout=layout)
        scan, dist, count = (t.cpu().numpy() for t in got[:3])
        assert (scan[1:] == -7.5).all() and (dist[1:] == 255).all() and count.tolist()[1:] == [0, 0] and count[0] > 0
        dev.fill(*_poses(pose[:, :3], pose[:, 3:], layout), iterations=4, filled_out=filled)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(filled), _bits(want[3])) and (want[4][1:] < 255).sum() > 100


def test_a_pose_far_from_the_window():
    """10 m from the origin with a 4 m window: every column lies outside, the row is unknown; the window fills all the same."""
    n, G = 2, 16
    dev, spec = _pair(n, G, unknown_value=1.5)
    _load(dev, spec, _random_maps(np.random.default_rng(5), n, G, 0.5), _origins(n, G))
    pos, quat = _near(spec)
    pos[0, 0] += 10.0
    pos[1, 1] -= 10.0
    got, want = _check(dev, spec, pos, quat, 8)
    assert (want[0] == 1.5).all() and (want[1] == 255).all() and not want[2].any() and (want[4] < 255).all()


def test_scan_into_the_columns_of_observation_rows():
    """scan_out aimed at columns 4 ... 964 of a (n + 1, 965) buffer (pitch 965, 4 bytes off): the four leading columns and the
    guard row keep their bits; so do guard bytes behind the column dist and the count."""
    n, G = 3, 32
    dev, spec = _pair(n, G)
    _load(dev, spec, _random_maps(np.random.default_rng(6), n, G, 0.05), _origins(n, G))
    pos, quat = _near(spec)
    rows = torch.full((n + 1, 965), GAP_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    dist = torch.full(((n + 1) * 961,), 77, dtype=torch.uint8, device="cuda")
    count = torch.full((n + 1,), -5, dtype=torch.int32, device="cuda")
    got, _ = _check(dev, spec, pos, quat, 6, scan_out=rows[:n, 4:], dist_out=dist[:n * 961].view(n, 961), count_out=count[:n])
    assert got[0].data_ptr() == rows.data_ptr() + 16 and got[0][1].data_ptr() % 16 == 4      # row 1 starts 4 bytes off
    raw = rows.view(torch.int32)
    assert (raw[:, :4] == GAP_BITS).all() and (raw[n] == GAP_BITS).all() and (dist[n * 961:] == 77).all() and count[n] == -5


def test_each_optional_output_null_in_turn():
    """Through the library: with one output NULL the others are what they are with all five; scan_out = NULL with filled_out given
    writes the window outputs only (and takes NULL ray tables)."""
    n, G = 3, 16
    dev, spec = _pair(n, G)
    _load(dev, spec, _random_maps(np.random.default_rng(7), n, G, 0.1), _origins(n, G))
    pos, quat = _near(spec)
    p, q = _poses(pos, quat, "aos")
    want = spec.fill(pos, quat, iterations=5)
    fc = _lib.ElevationFillCfg(5)
    sizes = ((n * 961, torch.float32), (n * 961, torch.uint8), (n, torch.int32), (n * G * G, torch.float32), (n * G * G, torch.uint8))

    def run(skip, rays=True):
        bufs = [torch.full((k + 1,), 99, dtype=dt, device="cuda") for k, dt in sizes]          # one guard element each
        ptrs = [None if i in skip else b.data_ptr() for i, b in enumerate(bufs)]
        _fused.launch("rover_elevation_fill", dev.map.device, dev.cfg, fc, p.data_ptr(), q.data_ptr(), p.stride(1), p.stride(0),
                      dev.map.data_ptr(), dev.origin.data_ptr(), dev.ray_x.data_ptr() if rays else None, dev.nx,
                      dev.ray_y.data_ptr() if rays else None, dev.ny, ptrs[0], 961, ptrs[1], ptrs[2], ptrs[3], ptrs[4], n)
        torch.cuda.synchronize()
        return bufs

    for skip, rays in (((), True), ((1,), True), ((2,), True), ((3,), True), ((4,), True), ((3, 4), True), ((1, 2, 4), True),
                       ((0,), True), ((0,), False), ((0, 4), False)):
        bufs = run(skip, rays)
        unwritten = set(skip) | ({1, 2} if 0 in skip else set())               # no scan: no column dist, no count
        for i, (b, w) in enumerate(zip(bufs, want)):
            assert b[-1] == 99, (skip, NAMES[i])
            if i in unwritten:
                assert (b == 99).all(), (skip, NAMES[i])
            else:
                assert np.array_equal(_bits(b[:-1]), _bits(w).reshape(-1)), (skip, NAMES[i])
    assert np.array_equal(_bits(dev.map), _bits(spec.map))


@pytest.mark.parametrize("size, res, grid", [((3.0, 3.0), 0.1, (31, 31)), ((1.0, 0.5), 0.25, (5, 3))])
def test_scanner_grids_and_measured_columns_equal_the_raw_scan(size, res, grid):
    """The default 31 x 31 scanner and a 5 x 3 one.  A column with dist 0 carries the bits rover_elevation_scan writes for the same
    map and pose, and dist is 0 exactly where that scan calls the column known."""
    n, G = 3, 32
    sc = RayCasterCfg(size=size, resolution=res)
    assert sc.grid == grid
    dev, spec = _pair(n, G, cell=0.1, scanner=sc, unknown_value=-2.0)
    _load(dev, spec, _random_maps(np.random.default_rng(8), n, G, 0.5), _origins(n, G))
    pos, quat = _near(spec, shift=(4.3, -2.4))
    got, _ = _check(dev, spec, pos, quat, 3)
    raw_scan, raw_known, raw_count = dev.scan(*_poses(pos, quat, "aos"))
    torch.cuda.synchronize()
    scan, dist, count = got[:3]
    assert scan.shape == (n, grid[0] * grid[1])
    measured = dist == 0
    assert torch.equal(measured, raw_known.bool()) and measured.any() and not measured.all()
    assert torch.equal(scan.view(torch.int32)[measured], raw_scan.view(torch.int32)[measured])
    assert (count >= raw_count).all() and (count > raw_count).any()


def test_the_class_refuses_what_it_cannot_pass_on():
    n, G = 2, 16
    dev, spec = _pair(n, G)
    pos, quat = _near(spec)
    p, q = _poses(pos, quat, "aos")
    for bad in (dict(iterations=0), dict(iterations=255), dict(filled_out=torch.empty(n, G, G)),
                dict(filled_out=torch.empty(n, G, G + 1, device="cuda")), dict(cell_dist_out=torch.empty(n, G, G, device="cuda")),
                dict(dist_out=torch.empty(n, 961, device="cuda")), dict(count_out=torch.empty(n + 1, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            dev.fill(p, q, **bad)
    out = dev.fill(p, q)                               # the cfg's fill_iterations; no window outputs unless asked for
    torch.cuda.synchronize()
    assert out[3] is None and out[4] is None and (out[1] == 255).all() and not out[2].any()
    assert C.sizeof(_lib.ElevationFillCfg) == _lib.load().rover_elevation_fill_cfg_bytes()
