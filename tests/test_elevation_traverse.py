"""The elevation map's slope / step / roughness / cost layers on the CPU (include/rover_elevation_traverse.h,
isaac_rover_orbit_amd.elevation): TorchElevationMap.traverse, the specification, against a cell-by-cell loop on np.float32 scalars;
an exact plane; a step edge; the gradient's fallbacks; support; the seam; class and cost; a plane seen through the real camera;
every refusal of the library (no GPU needed: the arguments are checked before the device is looked at) and of the cfg class; the
rig; the example's flags; the kernels' resources from the code object."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import elevation_cases as cases
from isaac_rover_orbit_amd import _lib
from isaac_rover_orbit_amd.cfg import CameraCfg, ElevationMapCfg, RayCasterCfg, RoverEnvCfg, TraverseCfg
from isaac_rover_orbit_amd.elevation import TorchElevationMap
from test_elevation_fill import _PLANE_POSES, _cell, _put_window, _window_of, f32, plane_map  # noqa: F401  (plane_map: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAN = math.nan
BIG = dict(slope_crit=1e30, step_crit=1e30, rough_crit=1e30)      # thresholds nothing finite and sane reaches


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    """Bit-equal, but that any NaN equals any NaN (float layers); plain equality for integer arrays."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)])


def _key(v) -> int:
    b = int(np.float32(v).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def layers_by_hand(h, t, cell, inv_cell):
    """Steps 2 and 3 of the header on the window `h` (G x G np.float32, window order), one cell at a time, every operation on
    np.float32 scalars in the header's order.  Returns (slope, step, rough, cost: G x G float32, NaN = no verdict; class: uint8)."""
    G = h.shape[0]
    r = t.radius
    cell, inv_cell = F(cell), F(inv_cell)
    out = [np.full((G, G), np.nan, F) for _ in range(4)]
    cls = np.zeros((G, G), np.uint8)
    ok = lambda i, j: 0 <= i < G and 0 <= j < G and bool(np.isfinite(h[i, j]))      # noqa: E731

    def gradient(lower, upper, centre):
        lo_ok, up_ok = ok(*lower), ok(*upper)
        if lo_ok and up_ok:
            return (h[upper] - h[lower]) * (F(0.5) * inv_cell)
        if up_ok:
            return (h[upper] - centre) * inv_cell
        if lo_ok:
            return (centre - h[lower]) * inv_cell
        return F(0.0)

    with np.errstate(all="ignore"):
        for i in range(G):
            for j in range(G):
                if not ok(i, j):
                    continue
                hc = h[i, j]
                near = [(di, dj) for di in range(-r, r + 1) for dj in range(-r, r + 1) if ok(i + di, j + dj)]
                support = len(near)
                if support < t.min_support:
                    continue
                vals = [h[i + di, j + dj] for di, dj in near]
                step = max(vals, key=_key) - min(vals, key=_key)
                gx, gy = gradient((i, j - 1), (i, j + 1), hc), gradient((i - 1, j), (i + 1, j), hc)
                slope = np.sqrt((gx * gx) + (gy * gy))
                acc = F(0.0)
                for di, dj in near:
                    if di or dj:
                        res = (h[i + di, j + dj] - hc) - ((gx * (F(dj) * cell)) + (gy * (F(di) * cell)))
                        acc = acc + res * res
                cnt = support - 1
                rough = np.sqrt(acc / F(cnt)) if cnt else F(0.0)
                lethal = not (slope < F(t.slope_crit) and step < F(t.step_crit) and rough < F(t.rough_crit))
                if lethal:
                    cost = F(1.0)
                else:
                    total = ((F(t.w_slope) * (slope / F(t.slope_crit))) + (F(t.w_step) * (step / F(t.step_crit)))) + \
                        (F(t.w_rough) * (rough / F(t.rough_crit)))
                    cost = total if total < F(1.0) else F(1.0)
                for layer, v in zip(out, (slope, step, rough, cost)):
                    assert isinstance(v, np.float32)
                    layer[i, j] = v
                cls[i, j] = 2 if lethal else 1
    return (*out, cls)


def columns_by_hand(c, ray_x, ray_y, origin, pos, quat):
    """Step 8's look-up on Python floats: per column the window cell (i, j) under it, or None (outside, or a bad pose)."""
    G = c.grid
    n_cols = len(ray_x) * len(ray_y)
    if not all(math.isfinite(v) for v in (*pos, *quat)):
        return [None] * n_cols
    px, py, _ = pos
    w, x, y, z = quat
    lo = (origin[0] - G // 2, origin[1] - G // 2)
    a = f32(1 - f32(2 * f32(f32(y * y) + f32(z * z))))
    b = f32(2 * f32(f32(w * z) + f32(x * y)))
    inv = f32(1 / f32(math.sqrt(f32(f32(a * a) + f32(b * b)))))
    cyaw, syaw = f32(a * inv), f32(b * inv)
    out = []
    for oy in ray_y:
        for ox in ray_x:
            sx_ = f32(px + f32(f32(cyaw * ox) - f32(syaw * oy)))
            sy_ = f32(py + f32(f32(syaw * ox) + f32(cyaw * oy)))
            gx, gy = _cell(sx_, c.inv_cell), _cell(sy_, c.inv_cell)
            out.append((gy - lo[1], gx - lo[0]) if (lo[0] <= gx < lo[0] + G and lo[1] <= gy < lo[1] + G) else None)
    return out


def _spec(G, n=1, cell=0.25, traverse=None, **kw):
    ecfg, cam, sc = cases.cfgs(12, 16, G, cell=cell, traverse=traverse or TraverseCfg(), **kw)
    return TorchElevationMap(ecfg, cam, sc, n)


def _window_layers(spec, window, origin=(-3, 5), cfg=None, e=0):
    """The five window results of env `e` for `window` (G x G, window order), back in window order."""
    _put_window(spec, e, window, origin)
    res = spec.traverse_window(cfg=cfg)
    return [_window_of(spec, e, a).astype(a.dtype) for a in res]


SPECIAL = np.array([-0.0, 0.0, 1e-42, -1e-42, 3e38, -3e38, np.inf, -np.inf], F)      # +-0, denormals, near the maximum, +-inf


def random_window(rng, G, known):
    h = rng.standard_normal((G, G)).astype(F)
    sp = rng.random((G, G)) < 0.06
    h[sp] = SPECIAL[rng.integers(0, len(SPECIAL), sp.sum())]
    if known == "one":
        mask = np.zeros((G, G), bool)
        mask[rng.integers(G), rng.integers(G)] = True
    else:
        mask = rng.random((G, G)) < known
    h[~mask] = np.nan
    return h


@pytest.mark.parametrize("known", [0.0, "one", 0.05, 0.5, 1.0])
@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("G", [8, 16])
def test_spec_against_a_cell_by_cell_loop(G, r, known):
    """Three envs with different windows and origins (negative, lo no multiple of G); the four layers, the class window, the cost
    scan, the column classes and the lethal count against the loops above, with min_support 1 and again with more (the full
    neighbourhood on the fully known windows).  With
    cell = 0.25 the 3 m scan leaves the 2 m window at G = 8; the special values overflow and make NaNs on the way."""
    n = 3
    t = TraverseCfg(radius=r, min_support=1, slope_crit=6.0, step_crit=5.0, rough_crit=3.0, w_slope=0.3, w_step=0.45, w_rough=0.25,
                    unknown_cost=-7.5)
    spec = _spec(G, n, traverse=t)
    c = spec.cfg
    rx, ry = [float(v) for v in spec.ray_x], [float(v) for v in spec.ray_y]
    rng = np.random.default_rng(1000 * G + 10 * r + (7 if known == "one" else int(known * 20)))
    origins = [(-3, 5), (G + 1, -2 * G - 3), (0, 0)]
    windows = [random_window(rng, G, known) for _ in range(n)]
    for e in range(n):
        _put_window(spec, e, windows[e], origins[e])
    pos = np.array([[(o[0] + 0.3) * 0.25, (o[1] + 0.6) * 0.25, 0.3 + 0.1 * e] for e, o in enumerate(origins)], F)
    quat = np.stack([cases.quat(0.4 + 1.9 * e, 0.03, -0.02) for e in range(n)])
    before = spec.map.copy(), spec.origin.copy()
    classes = set()
    for cfg in (t, TraverseCfg(**{**t.__dict__, "min_support": (2 * r + 1) ** 2 if known == 1.0 else 2})):
        scan, col_cls, count, slope, step, rough, cost = spec.traverse(pos, quat, cfg=cfg)
        cls = spec.traverse_window(cfg=cfg)[4]
        assert scan.dtype == slope.dtype == step.dtype == rough.dtype == cost.dtype == np.float32
        assert col_cls.dtype == cls.dtype == np.uint8 and count.dtype == np.int32 and scan.shape == (n, 961) and cost.shape == (n, G, G)
        for e in range(n):
            want = layers_by_hand(windows[e], cfg, c.cell, c.inv_cell)
            for got, w, nm in zip((slope, step, rough, cost, cls), want, ("slope", "step", "rough", "cost", "class")):
                assert _same(_window_of(spec, e, got).astype(w.dtype), w), (cfg.min_support, e, nm)
            under = columns_by_hand(c, rx, ry, origins[e], [float(v) for v in pos[e]], [float(v) for v in quat[e]])
            want_cls = [0 if ij is None else int(want[4][ij]) for ij in under]
            want_scan = np.array([want[3][ij] if k else F(-7.5) for ij, k in zip(under, want_cls)], F)
            assert col_cls[e].tolist() == want_cls and np.array_equal(_bits(scan[e]), _bits(want_scan)) and count[e] == want_cls.count(2)
            assert not np.isnan(scan[e]).any()
            classes |= set(want_cls)
    assert np.array_equal(_bits(spec.map), _bits(before[0])) and np.array_equal(spec.origin, before[1])      # read only
    assert classes == ({0} if known == 0.0 else {0, 1, 2} if known in (0.5, 1.0) else classes) and 0 in classes


def _plane(G, cell, a, b, c):
    j, i = np.meshgrid(np.arange(G), np.arange(G))
    return (F(a) * (j.astype(F) * F(cell)) + F(b) * (i.astype(F) * F(cell)) + F(c)).astype(F)


@pytest.mark.parametrize("r", [1, 2, 4])
def test_an_exact_plane(r):
    """h = 0.5 x - 0.25 y + 3 at cell = 0.125: every operation is exact.  The slope has the bits of sqrt(float32(0.3125)) in every
    cell, the borders included (one-sided differences agree on a plane); the roughness is exactly 0; the interior step is exactly
    2 r cell (|a| + |b|)."""
    G, cell = 16, 0.125
    spec = _spec(G, cell=cell, traverse=TraverseCfg(radius=r, **BIG))
    slope, step, rough, cost, cls = _window_layers(spec, _plane(G, cell, 0.5, -0.25, 3.0))
    assert (_bits(slope) == _bits(np.sqrt(F(0.3125)))).all()
    assert (_bits(rough) == 0).all()                                         # +0.0
    inner = step[r:G - r, r:G - r]
    assert (inner == F(2 * r * cell * 0.75)).all() and (r != 2 or (inner == F(0.375)).all())
    assert (step[0, 0] == F(r * cell * 0.75)) and (cls == 1).all() and (cost < 1e-20).all()


def test_a_step_edge():
    """A 0.25 m step between columns 7 and 8 at cell = 0.125, r = 2: step is 0.25 in exactly the four columns within r of the edge
    and 0 elsewhere; slope is 1.0 in the two columns beside the edge and 0 elsewhere; rough is non-zero only in those four."""
    G, cell = 16, 0.125
    spec = _spec(G, cell=cell, traverse=TraverseCfg(radius=2, **BIG))
    window = np.zeros((G, G), F)
    window[:, 8:] = 0.25
    slope, step, rough, cost, cls = _window_layers(spec, window)
    near = np.zeros((G, G), bool)
    near[:, 6:10] = True
    beside = np.zeros((G, G), bool)
    beside[:, 7:9] = True
    assert (step[near] == F(0.25)).all() and (step[~near] == 0).all()
    assert (slope[beside] == F(1.0)).all() and (slope[~beside] == 0).all()
    assert (rough[near] > 0).all() and (rough[~near] == 0).all() and (cls == 1).all()


def test_the_gradient_falls_back_to_one_side_and_to_zero():
    """A row 1, 2, 4, 8, ... along x with holes: centred where both neighbours are usable, one-sided towards the usable one (an inf
    is not usable), zero with neither; the same along y; the window's border is a missing neighbour."""
    G, cell = 8, 0.5
    spec = _spec(G, cell=cell, traverse=TraverseCfg(radius=1, **BIG))
    window = np.full((G, G), np.nan, F)
    window[3, :] = [1.0, 2.0, 4.0, NAN, 16.0, np.inf, 64.0, 128.0]
    slope = _window_layers(spec, window)[0]
    # gy = 0 everywhere (no usable cell above or below); inv_cell = 2
    assert slope[3].tolist()[:3] == [2.0, 3.0, 4.0]          # border: upper only (2 - 1) * 2; both: (4 - 1) * (0.5 * 2); lower only
    assert math.isnan(slope[3, 3]) and slope[3, 4] == 0.0 and math.isnan(slope[3, 5])        # neither side: 0
    assert slope[3, 6] == 128.0 and slope[3, 7] == 128.0     # upper only (128 - 64) * 2; the border: lower only
    slope_t = _window_layers(spec, window.T.copy())[0]
    assert _same(slope_t, slope.T.copy())
    both = np.full((G, G), np.nan, F)
    both[2:5, 2:5] = [[0.0, 1.0, 0.0], [3.0, 5.0, 9.0], [0.0, 2.0, 0.0]]
    assert _window_layers(spec, both)[0][3, 3] == np.sqrt(F((6.0 * 1.0) ** 2 + (1.0 * 1.0) ** 2))        # gx = 6, gy = 1


def test_support_an_isolated_cell_has_no_verdict():
    G = 8
    window = np.full((G, G), np.nan, F)
    window[4, 4] = 1.5
    for need, want in ((1, 1), (2, 0), (9, 0)):
        spec = _spec(G, traverse=TraverseCfg(radius=1, min_support=need))
        slope, step, rough, cost, cls = _window_layers(spec, window)
        assert cls[4, 4] == want and cls.sum() == want
        if want:
            assert (slope[4, 4], step[4, 4], rough[4, 4], cost[4, 4]) == (0.0, 0.0, 0.0, 0.0)      # no neighbour: g = 0, cnt = 0
        else:
            assert all(np.isnan(a).all() and (_bits(a) == 0x7FC00000).all() for a in (slope, step, rough, cost))
    full = np.ones((G, G), F)
    cls = _window_layers(_spec(G, traverse=TraverseCfg(radius=1, min_support=9)), full)[4]
    assert (cls[1:-1, 1:-1] == 1).all() and cls[0].sum() == 0 and cls[:, -1].sum() == 0      # the border lacks neighbours


def test_the_seam_is_no_neighbourhood():
    """The seam case of the fill: window (3, 0) of a window with low corner (-11, -3) and (3, G - 1), the adjacent SLOT across the
    seam, hold different heights: neither sees the other (support 1, step 0, slope 0)."""
    G = 16
    spec = _spec(G, traverse=TraverseCfg(radius=2, **BIG))
    window = np.full((G, G), np.nan, F)
    window[3, 0], window[3, G - 1] = 2.5, -4.0
    slope, step, rough, cost, cls = _window_layers(spec, window, origin=(-3, 5))
    assert tuple(spec.origin[0] - G // 2) == (-11, -3)
    for j in (0, G - 1):
        assert (cls[3, j], slope[3, j], step[3, j], rough[3, j]) == (1, 0.0, 0.0, 0.0)
    assert cls.sum() == 2
    assert _window_layers(_spec(G, traverse=TraverseCfg(radius=2, min_support=2)), window, origin=(-3, 5))[4].sum() == 0


def test_class_and_cost():
    G, cell = 16, 0.125
    up = lambda v: float(np.nextafter(F(v), F(np.inf)))      # noqa: E731
    plane, edge = _plane(G, cell, 0.5, -0.25, 3.0), np.zeros((G, G), F)
    edge[:, 8:] = 0.25
    s0 = float(np.sqrt(F(0.3125)))
    # the slope alone, at the threshold itself (< is strict) and one ulp above it
    spec = _spec(G, cell=cell)
    big = dict(step_crit=1e30, rough_crit=1e30)
    assert (_window_layers(spec, plane, cfg=TraverseCfg(slope_crit=s0, **big))[4] == 2).all()
    slope, step, rough, cost, cls = _window_layers(spec, plane, cfg=TraverseCfg(slope_crit=up(s0), **big))
    assert (cls == 1).all() and (cost < 1.0).all() and (cost > 0.39).all()                   # a cost window can be lethal-free
    # the step alone
    near = np.zeros((G, G), bool)
    near[:, 6:10] = True
    big = dict(slope_crit=1e30, rough_crit=1e30)
    cls = _window_layers(spec, edge, cfg=TraverseCfg(step_crit=0.25, **big))[4]
    assert (cls[near] == 2).all() and (cls[~near] == 1).all()
    assert (_window_layers(spec, edge, cfg=TraverseCfg(step_crit=up(0.25), **big))[4] == 1).all()
    # the roughness alone: the threshold is the largest roughness of the window
    rough = _window_layers(spec, edge, cfg=TraverseCfg(**BIG))[2]
    top = float(rough.max())
    big = dict(slope_crit=1e30, step_crit=1e30)
    slope, step, rough2, cost, cls = _window_layers(spec, edge, cfg=TraverseCfg(rough_crit=top, **big))
    assert np.array_equal(cls == 2, rough == F(top)) and 0 < (cls == 2).sum() < G * G and (cost[cls == 2] == 1.0).all()
    assert (_window_layers(spec, edge, cfg=TraverseCfg(rough_crit=up(top), **big))[4] == 1).all()
    # neighbours at +3e38 and -3e38: the step overflows, which no threshold excuses
    huge = np.zeros((G, G), F)
    huge[5, 5], huge[5, 6] = 3e38, -3e38
    slope, step, rough, cost, cls = _window_layers(spec, huge, cfg=TraverseCfg(radius=1, slope_crit=3e38, step_crit=3e38, rough_crit=3e38))
    assert np.isinf(step[5, 5]) and cls[5, 5] == cls[5, 6] == cls[4, 4] == 2 and cls[0, 0] == 1 and cost[5, 5] == 1.0
    assert (cls[3:8, 3:9] == 2).sum() == 12 and (cls == 2).sum() == 12
    # the weights move the cost of a cell that is not lethal, and nothing else
    t1 = TraverseCfg(step_crit=0.5, slope_crit=1.0, rough_crit=1.0)           # lethal beside the edge (slope 1), free one column on
    t2 = TraverseCfg(step_crit=0.5, slope_crit=1.0, rough_crit=1.0, w_slope=0.1, w_step=0.2, w_rough=0.7)
    a, b = _window_layers(spec, edge, cfg=t1), _window_layers(spec, edge, cfg=t2)
    assert all(_same(x, y) for x, y in zip(a[:3], b[:3])) and np.array_equal(a[4], b[4]) and set(a[4].ravel()) == {1, 2}
    assert (a[3][a[4] == 2] == 1.0).all() and (b[3][b[4] == 2] == 1.0).all()
    free = a[4] == 1
    assert (a[3][free & near] != b[3][free & near]).all() and (free & near).sum() == 2 * G and (a[3][free & ~near] == 0).all()
    # unknown_cost reaches the columns outside the window and every column of a bad pose
    t = TraverseCfg(unknown_cost=-3.25)
    spec = _spec(8, 2, traverse=t)
    spec.map[...] = 1.0
    spec.origin[...] = [[-3, 5], [9, 2]]
    pos = np.array([[-0.7, 1.3, 0.3], [NAN, 0.6, 0.5]], F)
    quat = np.stack([cases.quat(0.4), cases.quat(-2.0)])
    scan, col_cls, count, *_ = spec.traverse(pos, quat)
    assert (scan[1] == -3.25).all() and not col_cls[1].any() and count.tolist() == [0, 0]
    assert 0 < (col_cls[0] == 1).sum() < 961 and (scan[0][col_cls[0] == 0] == -3.25).all() and (scan[0][col_cls[0] == 1] == 0.0).all()
    # heights= takes another window in the map's place; the map is only read
    other = np.full_like(spec.map, 2.0)
    other[0, 3, 3] = 9.0
    got = spec.traverse(pos, quat, heights=other)
    assert got[2][0] > 0 and (spec.map == 1.0).all() and (got[4][0] > 0).sum() == 25
    with pytest.raises(ValueError):
        spec.traverse(pos, quat, heights=other[:1])
    with pytest.raises(ValueError):
        TorchElevationMap(ElevationMapCfg(), CameraCfg(), RayCasterCfg(), 1).traverse_window()         # no TraverseCfg anywhere


def test_a_plane_through_the_real_camera(plane_map):
    """The plane of the map's own test at its twelve poses, default TraverseCfg.  Without a fill every column of the 91-column
    corridor is class 1; with 16 sweeps (which fill all 961 columns at those poses) all 961 are.  The map's heights lie within
    eps = 8 ulp of 5 m of the plane (asserted here on the cells), so a height difference is at most 2 eps: with the centred
    difference the gradient is at most eps / cell per axis, slope <= sqrt(2) eps / cell; step <= 2 eps; a residual is at most
    2 eps + 2 (r cell)(eps / cell), so rough <= 2 eps (1 + r)."""
    c, sc, spec, p, q, _ = plane_map
    t = TraverseCfg()
    cell, r = float(spec.map_cfg.cell), t.radius
    eps = 8 * float(np.spacing(F(5.0)))
    front, _ = cases.corridor(sc)
    known = np.isfinite(spec.map)
    assert np.abs(spec.map[known].astype(np.float64) - c).max() <= eps
    bounds = (math.sqrt(2) * eps / cell, 2 * eps, 2 * eps * (1 + r))
    for heights, columns in ((None, front), (spec.fill(p, q, iterations=16)[3], np.ones(961, bool))):
        scan, col_cls, count, slope, step, rough, cost = spec.traverse(p, q, heights=heights, cfg=t)
        assert (col_cls[:, columns] == 1).all() and not count.any() and not (col_cls == 2).any()
        judged = ~np.isnan(cost)
        seen = [float(a[judged].max()) for a in (slope, step, rough)]
        print(f"{'map' if heights is None else 'filled'}: slope <= {seen[0]:.2e} (bound {bounds[0]:.2e}), step <= {seen[1]:.2e} "
              f"({bounds[1]:.2e}), rough <= {seen[2]:.2e} ({bounds[2]:.2e}); {judged.sum(axis=(1, 2)).min()} cells judged at the least")
        assert all(s <= b for s, b in zip(seen, bounds))
        top = t.w_slope * bounds[0] / t.slope_crit + t.w_step * bounds[1] / t.step_crit + t.w_rough * bounds[2] / t.rough_crit
        assert float(cost[judged].max()) <= top * (1 + 1e-6) and float(scan[:, columns].max()) <= top * (1 + 1e-6)
        assert (scan[col_cls == 0] == 1.0).all()                             # unknown_cost


def test_every_refusal_through_the_library():
    lib = _lib.load()
    assert lib.rover_elevation_traverse_cfg_bytes() == C.sizeof(_lib.ElevationTraverseCfg) == 36
    buf = np.zeros(8192, np.float32)
    base = buf.ctypes.data                               # never read or written: every call below is refused
    nan, inf = math.nan, math.inf
    MAP, ORG, POSE, RX, RY, SCAN, CLS, COUNT, SLOPE, STEP, ROUGH, COST = (
        base + 4 * o for o in (0, 512, 2816, 2880, 2912, 3072, 4096, 4160, 4608, 5120, 5632, 6144))

    def native(**kw):
        c = ElevationMapCfg(grid=16, cell=0.25).to_native((0.1, 0.0, 0.7), 0.25)
        for k, v in kw.items():
            if k == "mount_pos":
                for i in range(3):
                    c.mount_pos[i] = v[i]
            else:
                setattr(c, k, v)
        return c

    def tcfg(**kw):
        t = TraverseCfg().to_native()
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def run(cfg=None, null_cfg=False, t=None, null_t=False, pos=POSE, quat=POSE + 12, cs=1, es=7, mp=MAP, org=ORG, rx=RX, nx=5, ry=RY,
            ny=4, scan=SCAN, sp=20, cls=CLS, count=COUNT, slope=SLOPE, step=STEP, rough=ROUGH, cost=COST, n=2):
        cfg = cfg if cfg is not None else native()
        t = t if t is not None else tcfg()
        rc = lib.rover_elevation_traverse(None if null_cfg else C.byref(cfg), None if null_t else C.byref(t), pos, quat, cs, es, mp, org,
                                          rx, nx, ry, ny, scan, sp, cls, count, slope, step, rough, cost, n, None)
        return rc, lib.rover_last_error().decode()

    no_window = dict(slope=None, step=None, rough=None, cost=None)
    invalid = [
        (dict(null_cfg=True), "NULL"), (dict(null_t=True), "NULL"), (dict(pos=None), "NULL"), (dict(quat=None), "NULL"),
        (dict(mp=None), "NULL"), (dict(org=None), "NULL"), (dict(rx=None), "NULL"), (dict(ry=None), "NULL"),
        (dict(scan=None, **no_window), "NULL"), (dict(scan=None, rx=None, ry=None, **no_window), "NULL"),
        (dict(rx=None, **no_window), "NULL"), (dict(scan=None, mp=None), "NULL"),
        (dict(t=tcfg(radius=0)), "radius"), (dict(t=tcfg(radius=5)), "radius"), (dict(t=tcfg(radius=-1)), "radius"),
        (dict(t=tcfg(min_support=0)), "min_support"), (dict(t=tcfg(min_support=26)), "min_support"),
        (dict(t=tcfg(radius=1, min_support=10)), "min_support"), (dict(t=tcfg(min_support=-3)), "min_support"),
        (dict(t=tcfg(slope_crit=0.0)), "crit"), (dict(t=tcfg(slope_crit=inf)), "crit"), (dict(t=tcfg(slope_crit=nan)), "crit"),
        (dict(t=tcfg(step_crit=-0.1)), "crit"), (dict(t=tcfg(step_crit=nan)), "crit"), (dict(t=tcfg(step_crit=inf)), "crit"),
        (dict(t=tcfg(rough_crit=0.0)), "crit"), (dict(t=tcfg(rough_crit=nan)), "crit"), (dict(t=tcfg(rough_crit=-inf)), "crit"),
        (dict(t=tcfg(w_slope=-0.1)), "w_slope"), (dict(t=tcfg(w_step=nan)), "w_slope"), (dict(t=tcfg(w_rough=inf)), "w_slope"),
        (dict(t=tcfg(w_slope=0.5, w_step=0.5, w_rough=0.01)), "sum"), (dict(t=tcfg(w_slope=1.0000001, w_step=0.0, w_rough=0.0)), "sum"),
        (dict(t=tcfg(unknown_cost=nan)), "unknown_cost"),
        (dict(n=0), "n must"), (dict(n=-3), "n must"), (dict(nx=0), "nx and ny"), (dict(ny=-1), "nx and ny"),
        (dict(scan=None, nx=0), "nx and ny"), (dict(cs=0), "stride"), (dict(es=-7), "stride"),
        (dict(pos=POSE + 2), "aligned"), (dict(quat=POSE + 13), "aligned"), (dict(mp=MAP + 1), "aligned"), (dict(org=ORG + 2), "aligned"),
        (dict(rx=RX + 3), "aligned"), (dict(ry=RY + 1), "aligned"), (dict(scan=SCAN + 2), "aligned"), (dict(count=COUNT + 1), "aligned"),
        (dict(slope=SLOPE + 2), "aligned"), (dict(step=STEP + 1), "aligned"), (dict(rough=ROUGH + 3), "aligned"),
        (dict(cost=COST + 2), "aligned"),
        (dict(sp=19), "scan_pitch"),
        (dict(cfg=native(cell=0.0)), "cell"), (dict(cfg=native(cell=inf)), "cell"), (dict(cfg=native(cell=nan)), "cell"),
        (dict(cfg=native(inv_cell=-4.0)), "cell"), (dict(cfg=native(inv_cell=nan)), "cell"), (dict(cfg=native(inv_cell=inf)), "cell"),
        (dict(cfg=native(range_min=0.0)), "range_min"), (dict(cfg=native(range_min=nan)), "range_min"),
        (dict(cfg=native(range_min=2.0, range_max=1.0)), "range_max"), (dict(cfg=native(range_max=nan)), "range_max"),
        (dict(cfg=native(alpha=0.0)), "alpha"), (dict(cfg=native(alpha=1.5)), "alpha"), (dict(cfg=native(alpha=nan)), "alpha"),
        (dict(cfg=native(unknown_value=nan)), "unknown_value"), (dict(cfg=native(height_offset=nan)), "height_offset"),
        (dict(cfg=native(mount_pos=(0.0, inf, 0.0))), "mount_pos"),
        (dict(scan=MAP + 4 * 100), "overlap"), (dict(mp=SCAN + 4 * 39), "overlap"), (dict(mp=SCAN - 4 * 511), "overlap"),
        (dict(slope=MAP + 4 * 511), "overlap"), (dict(step=MAP - 4 * 511), "overlap"), (dict(rough=MAP), "overlap"),
        (dict(cost=MAP + 4 * 8), "overlap"), (dict(cls=MAP + 100), "overlap"), (dict(cls=MAP - 39), "overlap"),
        (dict(count=MAP + 4 * 511), "overlap"), (dict(count=MAP - 4), "overlap"),
    ]
    for kw, text in invalid:
        rc, msg = run(**kw)
        assert rc == 1 and msg.startswith("rover_elevation_traverse:") and text in msg, (kw, rc, msg)
    for kw, text in ((dict(cfg=native(grid=4)), "power of two"), (dict(cfg=native(grid=256)), "power of two"),
                     (dict(cfg=native(grid=24)), "power of two"), (dict(cfg=native(grid=0)), "power of two"),
                     (dict(nx=65, ny=64, sp=65 * 64), "4096"), (dict(scan=None, nx=65, ny=64), "4096")):
        rc, msg = run(**kw)
        assert rc == 4 and msg.startswith("rover_elevation_traverse:") and text in msg, (kw, rc, msg)
    assert not buf.any()
    # on a host without a GPU, what is allowed gets past the argument checks and fails at the device query, with nothing written
    allowed = () if torch.cuda.is_available() else (
        dict(), dict(**no_window), dict(scan=None, rx=None, ry=None), dict(scan=None, cls=None, count=None, slope=None, step=None, rough=None),
        dict(cls=None, count=None), dict(t=tcfg(radius=4, min_support=81)), dict(t=tcfg(radius=1, min_support=9)),
        dict(t=tcfg(w_slope=0.0, w_step=0.0, w_rough=0.0, unknown_cost=-inf)), dict(t=tcfg(w_slope=1.0, w_step=0.0, w_rough=0.0)),
        dict(cfg=native(range_max=inf, unknown_value=-inf, grid=8)), dict(cs=2, es=1), dict(slope=MAP + 4 * 512), dict(cls=MAP - 40),
        dict(count=MAP - 8), dict(slope=STEP, rough=STEP))
    for kw in allowed:
        rc, msg = run(**kw)
        assert rc != 0 and not msg.startswith("rover_elevation_traverse:"), (kw, rc, msg)
    assert not buf.any()


def test_the_cfg_class_checks_the_traverse():
    d = TraverseCfg()
    assert (d.radius, d.min_support, d.slope_crit, d.step_crit, d.rough_crit) == (2, 1, 0.577, 0.3, 0.1)
    assert (d.w_slope, d.w_step, d.w_rough, d.unknown_cost) == (0.4, 0.4, 0.2, 1.0) and ElevationMapCfg().traverse is None
    d.check()
    nan, inf = math.nan, math.inf
    for bad in (dict(radius=0), dict(radius=5), dict(radius=2.0), dict(radius=True), dict(radius="2"), dict(min_support=0),
                dict(min_support=26), dict(radius=1, min_support=10), dict(min_support=1.0), dict(slope_crit=0.0), dict(slope_crit=inf),
                dict(step_crit=nan), dict(step_crit=-1.0), dict(rough_crit=0.0), dict(rough_crit=1e39), dict(w_slope=-0.1),
                dict(w_step=nan), dict(w_rough=inf), dict(w_slope=0.5, w_step=0.5, w_rough=0.01), dict(w_slope=1.0000001, w_step=0, w_rough=0),
                dict(unknown_cost=nan)):
        with pytest.raises(ValueError):
            TraverseCfg(**bad).check()
    for good in (dict(radius=1, min_support=9), dict(radius=4, min_support=81), dict(w_slope=0.0, w_step=0.0, w_rough=0.0),
                 dict(w_slope=1.0, w_step=0.0, w_rough=0.0), dict(unknown_cost=-inf), dict(unknown_cost=0.0),
                 dict(w_slope=1.00000001, w_step=0.0, w_rough=0.0)):       # 1 in fp32
        TraverseCfg(**good).check()
    t = TraverseCfg(radius=3, min_support=4, unknown_cost=0.5).to_native()
    assert (t.radius, t.min_support, t.unknown_cost, C.sizeof(t)) == (3, 4, 0.5, 36) and t.slope_crit == f32(0.577)
    cfg = RoverEnvCfg(camera=CameraCfg(), elevation=ElevationMapCfg(traverse=TraverseCfg(radius=7)))
    with pytest.raises(ValueError, match="radius"):
        cfg.validate()
    cfg.elevation.traverse.radius = 4
    cfg.validate()
    # the native struct of the map is what it was: the traverse parameters travel in a struct of their own
    c = ElevationMapCfg(traverse=TraverseCfg()).to_native(CameraCfg().position, 0.25)
    assert C.sizeof(c) == 44 and bytes(c) == bytes(ElevationMapCfg().to_native(CameraCfg().position, 0.25))


def test_the_rig_runs_traverse_behind_map_and_fill_and_not_by_default():
    """On the CPU over test_sensor_rig's stand-ins.  Default: no key, no buffers, and fill() gets today's keywords only (the stand-in
    of the fill's own test takes no others).  With traverse: map, fill, traverse behind every map launch (reset, steps, a reset with
    draws) on the map launch's pose; traverse reads the window the fill wrote where there is a fill and the map where there is none;
    its outputs rotate under the three new keys; the six older keys hold what their launches wrote."""
    import test_sensor_rig as rig_cases
    from isaac_rover_orbit_amd.envs._sensors import FILL_KEYS, KEYS, TRAVERSE_KEYS, SensorRig
    assert TRAVERSE_KEYS == ("elevation_cost", "elevation_cost_class", "elevation_lethal_count")
    assert not set(TRAVERSE_KEYS) & (set(KEYS) | set(FILL_KEYS))
    N, COLS, G = rig_cases.N, rig_cases.COLS, 8

    class TodaysFill(rig_cases.MapStandIn):
        def fill(self, pos, quat, scan_out=None, dist_out=None, count_out=None, iterations=None):      # exactly today's arguments
            self.log.append(("fill", {}))

    for fill_iterations in (0, 5):
        host, log = rig_cases.Host(), []
        rig = SensorRig(host, "cpu", N, pose=(torch.zeros(N, 3), torch.zeros(N, 4)), elevation=TodaysFill(log), map_source="lidar",
                        lidar=rig_cases.LidarStandIn(log), fill_iterations=fill_iterations)
        rig.update(force=True)
        assert rig.traverse is None and not hasattr(rig, "_costs") and not hasattr(rig, "_filled") and not set(TRAVERSE_KEYS) & set(host.extras)
        assert [nm for nm, _ in log if nm in ("map", "fill", "traverse")] == (["map", "fill"] if fill_iterations else ["map"])

    class FullMap(rig_cases.MapStandIn):
        grid = G

        def fill(self, pos, quat, scan_out=None, dist_out=None, count_out=None, iterations=None, filled_out=None):
            scan_out.fill_(500 + self.calls), dist_out.fill_(self.calls), count_out.fill_(10 + self.calls)
            filled_out.fill_(700 + self.calls)
            self.log.append(("fill", {"pos": pos, "quat": quat, "outs": (scan_out, dist_out, count_out), "filled_out": filled_out}))

        def traverse(self, pos, quat, heights=None, scan_out=None, class_out=None, count_out=None, cfg=None):
            scan_out.fill_(900 + self.calls), class_out.fill_(self.calls), count_out.fill_(20 + self.calls)
            self.log.append(("traverse", {"pos": pos, "quat": quat, "heights": heights, "outs": (scan_out, class_out, count_out), "cfg": cfg,
                                          "window": None if heights is None else float(heights[0, 0, 0])}))

    tc = TraverseCfg(radius=3, unknown_cost=0.75)
    for source, camera, fill_iterations in (("camera", True, 5), ("lidar", False, 5), ("camera", True, 0), ("lidar", False, 0)):
        host, log = rig_cases.Host(), []
        host.extras["elevation_cost"] = "stale"
        pose = (torch.zeros(N, 3), torch.zeros(N, 4))
        kw = dict(pose=pose, elevation=FullMap(log), map_source=source, unknown_value=-1.0, fill_iterations=fill_iterations, traverse=tc)
        if camera:
            kw.update(render=lambda cfg, ws, buf: buf.fill_(1.0), camera_cfg="camera-cfg", workspace="workspace", image=(rig_cases.H, rig_cases.W))
        else:
            kw.update(lidar=rig_cases.LidarStandIn(log))
        rig = SensorRig(host, "cpu", N, **kw)
        ex = host.extras
        assert ex["elevation_cost"].shape == (N, COLS) and ex["elevation_cost"].dtype == torch.float32 and bool((ex["elevation_cost"] == 0.75).all())
        assert ex["elevation_cost_class"].shape == (N, COLS) and ex["elevation_cost_class"].dtype == torch.uint8
        assert not bool(ex["elevation_cost_class"].any())
        assert ex["elevation_lethal_count"].dtype == torch.int32 and ex["elevation_lethal_count"].shape == (N,)
        assert set(KEYS[5:]) <= set(ex) and (set(FILL_KEYS) <= set(ex)) == bool(fill_iterations)
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
            names = [nm for nm, _ in log if nm in ("map", "fill", "traverse")]
            assert names == (["map", "fill", "traverse"] if fill_iterations else ["map", "traverse"]), (kind, names)
            m, t = dict(log)["map"], dict(log)["traverse"]
            assert t["pos"] is m["pos"] is pose[0] and t["quat"] is m["quat"] is pose[1] and t["cfg"] is tc
            if fill_iterations:
                f = dict(log)["fill"]
                assert f["filled_out"] is t["heights"] and t["heights"].shape == (N, G, G) and t["window"] == 700 + call
                assert all(o is ex[k] for o, k in zip(f["outs"], FILL_KEYS)) and bool((ex["elevation_scan_filled"] == 500 + call).all())
            else:
                assert t["heights"] is None                                  # the map itself
            assert all(o is ex[k] for o, k in zip(t["outs"], TRAVERSE_KEYS)) and all(o is ex[k] for o, k in zip(m["outs"], KEYS[5:]))
            assert bool((ex["elevation_cost"] == 900 + call).all()) and bool((ex["elevation_cost_class"] == call).all())
            assert bool((ex["elevation_lethal_count"] == 20 + call).all()) and bool((ex["elevation_scan"] == 300 + call).all())
            assert bool((ex["elevation_count"] == call).all())
            if previous is not None:                                         # the frame before this one was not written over
                assert all(o is not p for o, p in zip(t["outs"], previous[0])) and bool((previous[0][0] == previous[1]).all())
            previous = (t["outs"], 900 + call)
        assert set(rig.state_dict()) == {"elevation_map", "elevation_origin"}
        SensorRig(host)                                                      # a rig without sensors removes the keys
        assert not set(TRAVERSE_KEYS) & set(host.extras)


def test_example_flags_switch_the_cost_on():
    import importlib.util
    spec = importlib.util.spec_from_file_location("eval_policy_example_cost", os.path.join(ROOT, "examples", "03_eval_policy.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    ap = ex.build_parser()
    with pytest.raises(ValueError, match="--scan_source elevation"):
        ex.make_cfg(ap.parse_args(["--checkpoint", "x.pt", "--map_cost"]))
    plain = ex.make_cfg(ap.parse_args(["--checkpoint", "x.pt", "--scan_source", "elevation"]))
    assert plain.elevation.traverse is None and plain.elevation == ElevationMapCfg()
    for extra, source, fill in (([], "camera", "none"), (["--map_source", "lidar", "--map_fill", "min"], "lidar", "min")):
        cfg = ex.make_cfg(ap.parse_args(["--checkpoint", "x.pt", "--scan_source", "elevation", "--map_cost", *extra]))
        assert cfg.elevation.traverse == TraverseCfg() and (cfg.elevation.source, cfg.elevation.fill) == (source, fill)
        cfg.validate()
    cfg = ex.make_cfg(ap.parse_args(["--checkpoint", "x.pt", "--scan_source", "elevation", "--map_cost", "--map_cost_radius", "4"]))
    assert cfg.elevation.traverse == TraverseCfg(radius=4)
    bad = ex.make_cfg(ap.parse_args(["--checkpoint", "x.pt", "--scan_source", "elevation", "--map_cost", "--map_cost_radius", "5"]))
    with pytest.raises(ValueError, match="radius"):
        bad.validate()


def test_traverse_kernels_use_no_scratch_and_bounded_lds():
    """Each of the five instantiations of the dense kernel: no private segment, static LDS <= 8 G^2 + 512 bytes (the height image,
    the cost image and the wave counters are 8 G^2 + 32), 512 threads.  The sparse kernel, five more under a name of its own: no
    private segment, one image (<= 4 G^2 + 256), and few enough registers (<= 128) for two workgroups per CU and more."""
    from helpers import gfx950_code_objects
    from isaac_rover_orbit_amd import build
    build.build_extension()
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("ROCm llvm tools not installed")
    seen, sparse = {}, {}
    for blob in gfx950_code_objects(_lib.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True).stdout
        for entry in re.split(r"\n\s*- \.", notes):
            m = re.search(r"\.name:\s*(\S*elevation_traverse_(sparse_)?kernel\S*)", entry)
            if not m or ".private_segment_fixed_size" not in entry:
                continue
            assert not any(other in m.group(1) for other in ("elevation_step_kernel", "elevation_scan_kernel", "elevation_fill_kernel"))
            G = int(re.search(r"ILi(\d+)E", m.group(1)).group(1))
            assert re.search(r"\.private_segment_fixed_size:\s*0\b", entry), f"{m.group(1)} uses scratch memory"
            lds = int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", entry).group(1))
            assert re.search(r"\.max_flat_workgroup_size:\s*512\b", entry)
            if m.group(2):
                assert lds <= 4 * G * G + 256 and int(re.search(r"\.vgpr_count:\s*(\d+)", entry).group(1)) <= 128, (G, lds)
                sparse[G] = sparse.get(G, 0) + 1
            else:
                assert lds <= 8 * G * G + 512 and lds <= 160 * 1024, (G, lds)
                seen[G] = seen.get(G, 0) + 1
    assert seen == sparse == {8: 1, 16: 1, 32: 1, 64: 1, 128: 1}
