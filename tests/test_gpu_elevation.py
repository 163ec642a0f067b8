"""The rolling elevation map as one HIP launch on the MI355X (include/rover_elevation.h, isaac_rover_orbit_amd.elevation) against
TorchElevationMap, its CPU specification.

Everything here is BIT-EQUAL on map, origin, scan, known and count: the kernel is comparisons, integer cell arithmetic, an integer
maximum and correctly rounded fp32 operations in a fixed order with contraction off, and numpy float32 does the same, so equality
is derived, not measured.  The one tolerance test (the map against the oracle scan) is in tests/test_gpu_elevation_env.py.
"""
import numpy as np
import pytest
import torch

import elevation_cases as cases

pytestmark = pytest.mark.gpu

GAP_BITS = 0x7FC0BEEF                                  # a NaN with a payload: what the frames around the buffers hold


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _pair(n, H, W, G, rays=None, **kw):
    from isaac_rover_orbit_amd.elevation import ElevationMap, TorchElevationMap
    ecfg, cam, sc = cases.cfgs(H, W, G, **kw)
    return ElevationMap(ecfg, cam, sc, n, "cuda", rays=rays), TorchElevationMap(ecfg, cam, sc, n, rays=rays), cam


def _poses(pos, quat, layout):
    """(pos, quat) device views of one pose array: the env's SoA rows (component stride n) or an (n, 7) AoS array."""
    both = torch.from_numpy(np.concatenate([pos, quat], 1).astype(np.float32)).cuda()
    if layout == "soa":
        st = both.t().contiguous()                     # (7, n)
        return st[0:3].t(), st[3:7].t()
    return both[:, :3], both[:, 3:]


def _same(dev, spec, got, want, what=""):
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dev.map), _bits(spec.map)), f"{what}: map"
    assert np.array_equal(dev.origin.cpu().numpy(), spec.origin), f"{what}: origin"
    if got is not None and got[0] is not None:
        for g, w, nm in zip(got, want, ("scan", "known", "count")):
            assert np.array_equal(_bits(g).reshape(w.shape), _bits(w)), f"{what}: {nm}"


def _step(dev, spec, depth, pos, quat, reset=(None, None), layout="aos", what="", **outs):
    p, q = _poses(pos, quat, layout)
    d = None if depth is None else torch.from_numpy(depth).cuda()
    r = tuple(None if f is None else torch.from_numpy(np.asarray(f, np.uint8)).cuda() for f in reset)
    got = dev.update(d, p, q, reset=r, **outs)
    want = spec.update(depth, pos, quat, reset=reset)
    _same(dev, spec, got, want, what)
    return got, want


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_steps_across_cell_borders(alpha, layout):
    """3 envs, 12 x 16 image, G = 16: four consecutive steps on the map the step before wrote (in-place reuse), the poses crossing
    cell borders in +x / -y, -x, diagonally, at negative x, the yaw in every quadrant.  alpha = 1 writes the frame's maximum
    itself; alpha = 0.5 blends over the frames."""
    n, H, W, G = 3, 12, 16, 16
    dev, spec, cam = _pair(n, H, W, G, cell=0.25, alpha=alpha, unknown_value=-7.5)
    rng = np.random.default_rng(11)
    origins = []
    for s, (pos, quat) in enumerate(cases.walk(n, 4)):
        depth = cases.random_depth(rng, n, H * W, 0.4, 3.0)
        (_, known, count), _ = _step(dev, spec, depth, pos, quat, layout=layout, what=f"step {s}")
        origins.append(spec.origin.copy())
        assert (count.cpu().numpy() > 0).all() and (known.cpu().numpy().sum(1) == count.cpu().numpy()).all()
        valid, wx, wy, wz = spec.points(depth, *spec._pose(pos, quat)[:2])
        for e in range(n):                             # the frame's plain float maximum per cell, by a loop of its own
            lo = spec.origin[e].astype(np.int64) - G // 2
            gx, gy = spec.cells(wx[e]), spec.cells(wy[e])
            inside = valid[e] & (gx >= lo[0]) & (gx < lo[0] + G) & (gy >= lo[1]) & (gy < lo[1] + G)
            frame = {}
            for k in np.nonzero(inside)[0]:
                key = (int(gy[k]) & (G - 1), int(gx[k]) & (G - 1))
                frame[key] = max(frame.get(key, -np.inf), float(wz[e, k]))
            assert len(frame) > 10
            m = dev.map[e].cpu().numpy()
            for (sy, sx), f in frame.items():
                if alpha == 1.0 or s == 0:             # a cell the frame touched holds the frame's maximum itself
                    assert m[sy, sx] == np.float32(f)
    assert len({tuple(o.reshape(-1)) for o in origins}) == 4 and (np.array(origins)[:, :, 0] < 0).all()


def test_odd_image_pitch_offset_and_framed_scan():
    """5 envs, 7 x 9 = 63 pixels (no multiple of 4 or 64); the image pitch above height * width and the depth pointer 4 bytes off a
    16-byte boundary; the scan into columns 4 ... 964 of a (5, 965) buffer whose other columns keep their bits."""
    n, H, W, G = 5, 7, 9, 32
    dev, spec, cam = _pair(n, H, W, G, cell=0.25)
    pos, quat = cases.walk(n, 1)[0]
    depth = cases.random_depth(np.random.default_rng(3), n, H * W, 0.4, 3.5)
    pitch, lead = H * W + 6, 1
    flat = torch.full((lead + n * pitch,), GAP_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    view = flat[lead:].view(n, pitch)[:, :H * W]
    view.copy_(torch.from_numpy(depth))
    assert view.data_ptr() % 16 == 4
    rows = torch.full((n, 965), GAP_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    p, q = _poses(pos, quat, "aos")
    got = dev.update(view, p, q, scan_out=rows[:, 4:])
    want = spec.update(depth, pos, quat)
    _same(dev, spec, got, want)
    assert got[0].data_ptr() == rows.data_ptr() + 16 and (rows.view(torch.int32)[:, :4] == GAP_BITS).all()
    gap = flat.view(torch.int32)
    assert (gap[:lead] == GAP_BITS).all() and (gap[lead:].view(n, pitch)[:, H * W:] == GAP_BITS).all()
    assert np.array_equal(_bits(view), _bits(depth)) and want[2].min() > 0


def test_one_cell_under_full_contention():
    """2 envs, 64 x 64 image, G = 8, all 4096 rays identical: every point lands in one cell and the LDS maximum is contended by
    all of them.  The depths are distinct; env 0 has the largest first, env 1 has it last."""
    n, H, W, G = 2, 64, 64, 8
    ray = np.array([0.6, 0.0, 0.8], np.float32)        # upwards: the largest depth is the highest point
    rays = np.tile(ray, (H * W, 1))
    dev, spec, cam = _pair(n, H, W, G, rays=rays, cell=0.5, range_max=6.0)
    d = (2.0 + np.arange(H * W) * 2.0 ** -21).astype(np.float32)
    assert len(np.unique(d)) == H * W
    depth = np.stack([d[::-1], d]).copy()
    pos = np.array([[0.1, 0.1, 0.3], [-5.15, 3.1, 0.2]], np.float32)
    quat = np.stack([cases.quat(0.0), cases.quat(0.0)])
    _step(dev, spec, depth, pos, quat)
    m = dev.map.cpu().numpy()
    assert (np.isfinite(m).reshape(n, -1).sum(1) == 1).all()
    _, _, _, wz = spec.points(depth, *spec._pose(pos, quat)[:2])
    assert (m[np.isfinite(m)] == wz.max(1)).all() and (wz.max(1) > wz.min(1)).all()


def test_largest_grid_with_the_real_camera():
    """G = 128 (64 KiB of LDS) with the 160 x 90 camera over a plane, 2 envs, two frames."""
    n, G = 2, 128
    dev, spec, cam = _pair(n, 90, 160, G, range_max=8.0)
    for s, (pos, quat) in enumerate(cases.walk(n, 2, start=(-0.37, 0.21))):
        depth = cases.plane_depth(cam, pos, quat, ground=-0.05)
        (_, _, count), _ = _step(dev, spec, depth, pos, quat, what=f"frame {s}")
        assert (count.cpu().numpy() >= 91).all()
    assert (np.isfinite(spec.map).reshape(n, -1).sum(1) > 1000).all()


@pytest.mark.parametrize("move, kept_columns", [(16, 0), (15, 1), (-16, 0), (-15, 1), (1, 15)])
def test_seam_and_moves_of_a_whole_window(move, kept_columns):
    """The window lies across slot 0 on both axes (centre cell (0, -1)); then a move of exactly G, G - 1 and one cells along x
    without a frame (depth = None): nothing, one column and G - 1 columns of the window survive."""
    n, H, W, G = 2, 12, 16, 16
    dev, spec, cam = _pair(n, H, W, G, cell=0.25)
    full = np.random.default_rng(2).standard_normal((n, G, G)).astype(np.float32)
    pos = np.array([[0.05, -0.05, 0.3], [0.2, -0.2, 0.3]], np.float32)
    quat = np.stack([cases.quat(0.3), cases.quat(-2.0)])
    _step(dev, spec, None, pos, quat)                   # sets the origin
    assert (spec.origin == [[0, -1], [0, -1]]).all()
    dev.map.copy_(torch.from_numpy(full))
    spec.map[...] = full
    pos2 = pos + np.array([move * 0.25, 0.0, 0.0], np.float32)
    (_, _, _), _ = _step(dev, spec, None, pos2, quat, what="moved")
    assert (np.isfinite(dev.map.cpu().numpy()).reshape(n, -1).sum(1) == kept_columns * G).all()
    kept = np.isfinite(spec.map)
    assert np.array_equal(spec.map[kept].view(np.int32), full[kept].view(np.int32))


@pytest.mark.parametrize("use_a, use_b", [(True, False), (False, True), (True, True), (False, False)])
def test_reset_flags(use_a, use_b):
    """reset_a only, reset_b only, both, both NULL: only the flagged env's map starts over."""
    n, H, W, G = 4, 12, 16, 16
    dev, spec, cam = _pair(n, H, W, G, cell=0.25)
    rng = np.random.default_rng(8)
    pos, quat = cases.walk(n, 1)[0]
    _step(dev, spec, cases.random_depth(rng, n, H * W, 0.4, 3.0), pos, quat)
    before = spec.map.copy()
    a, b = np.array([0, 1, 0, 0], np.uint8), np.array([0, 0, 0, 1], np.uint8)
    _step(dev, spec, None, pos, quat, reset=(a if use_a else None, b if use_b else None))
    flagged = (a * use_a + b * use_b).astype(bool)
    m = dev.map.cpu().numpy()
    assert np.isnan(m[flagged]).all() and np.array_equal(m[~flagged].view(np.int32), before[~flagged].view(np.int32))
    assert np.isfinite(before).reshape(n, -1).any(1).all()
    _step(dev, spec, cases.random_depth(rng, n, H * W, 0.4, 3.0), pos, quat, reset=(a if use_a else None, b if use_b else None))


def test_depth_values_at_and_outside_the_range():
    """NaN, +-inf, 0, negative, above range_max, just outside both ends: dropped; exactly range_min and range_max: included.
    Twelve rays fan out so that every valid pixel has a cell of its own."""
    n, H, W, G = 1, 3, 4, 32
    az = np.deg2rad(np.arange(12) * 30.0)
    rays = np.stack([np.cos(az), np.sin(az), np.zeros(12)], 1).astype(np.float32)
    dev, spec, cam = _pair(n, H, W, G, rays=rays, cell=0.25, range_min=0.5, range_max=2.0)
    lo, hi = np.float32(0.5), np.float32(2.0)
    depth = np.array([[np.nan, np.inf, -np.inf, 0.0, -1.0, 2.5, lo, hi, 1.0, 1.5, np.nextafter(lo, np.float32(0)),
                       np.nextafter(hi, np.float32(9))]], np.float32)
    pos, quat = np.array([[0.1, 0.1, 0.3]], np.float32), cases.quat(0.0)[None]
    _step(dev, spec, depth, pos, quat)
    assert np.isfinite(dev.map.cpu().numpy()).sum() == 4


@pytest.mark.parametrize("flag", [False, True])
def test_bad_poses_leave_the_map_alone(flag):
    """NaN in pos.z only (env 1) and inf in one quaternion word (env 2): map and origin untouched (all NaN with the reset flag),
    the row unknown, the count 0; env 0 goes on as usual."""
    n, H, W, G = 3, 12, 16, 16
    dev, spec, cam = _pair(n, H, W, G, cell=0.25, unknown_value=-7.5)
    rng = np.random.default_rng(4)
    (pos, quat), (pos2, quat2) = cases.walk(n, 2)
    _step(dev, spec, cases.random_depth(rng, n, H * W, 0.4, 3.0), pos, quat)
    before, origin = spec.map.copy(), spec.origin.copy()
    pos2[1, 2], quat2[2, 1] = np.nan, np.inf
    reset = (np.ones(n, np.uint8), None) if flag else (None, None)
    (scan, known, count), _ = _step(dev, spec, cases.random_depth(rng, n, H * W, 0.4, 3.0), pos2, quat2, reset=reset)
    m = dev.map.cpu().numpy()
    assert np.array_equal(dev.origin.cpu().numpy()[1:], origin[1:]) and (dev.origin.cpu().numpy()[0] != origin[0]).any()
    if flag:
        assert np.isnan(m[1:]).all()
    else:
        assert np.array_equal(m[1:].view(np.int32), before[1:].view(np.int32)) and np.isfinite(before[1:]).any()
    assert (scan[1:] == -7.5).all() and not known[1:].any() and count.tolist()[1:] == [0, 0] and count[0] > 0


def test_scan_entry_equals_the_scan_half_of_step():
    """rover_elevation_scan for the step's poses gives the step's own bits and leaves map and origin alone; for other poses it
    equals the specification; a bad pose gives an unknown row."""
    n, H, W, G = 3, 12, 16, 32
    dev, spec, cam = _pair(n, H, W, G, cell=0.25, unknown_value=3.25)
    rng = np.random.default_rng(6)
    (pos, quat), (pos2, quat2) = cases.walk(n, 2)
    (scan, known, count), _ = _step(dev, spec, cases.random_depth(rng, n, H * W, 0.4, 3.5), pos, quat)
    m0, o0 = dev.map.clone(), dev.origin.clone()
    for layout in ("aos", "soa"):
        again = dev.scan(*_poses(pos, quat, layout))
        torch.cuda.synchronize()
        for a, b in zip(again, (scan, known, count)):
            assert np.array_equal(_bits(a), _bits(b))
    pos2[2, 0] = np.inf
    rows = torch.full((n, 965), GAP_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    got = dev.scan(*_poses(pos2, quat2, "aos"), scan_out=rows[:, 4:])
    _same(dev, spec, got, spec.scan(pos2, quat2))
    assert (rows.view(torch.int32)[:, :4] == GAP_BITS).all() and (got[0][2] == 3.25).all() and got[2].tolist()[2] == 0
    assert torch.equal(dev.map.view(torch.int32), m0.view(torch.int32)) and torch.equal(dev.origin, o0)


def test_checkpoint_and_clear():
    n, H, W, G = 2, 12, 16, 16
    dev, spec, cam = _pair(n, H, W, G, cell=0.25)
    pos, quat = cases.walk(n, 1)[0]
    _step(dev, spec, cases.random_depth(np.random.default_rng(1), n, H * W, 0.4, 3.0), pos, quat)
    other, _, _ = _pair(n, H, W, G, cell=0.25)
    other.load_state_dict(dev.state_dict())
    assert torch.equal(other.map.view(torch.int32), dev.map.view(torch.int32)) and torch.equal(other.origin, dev.origin)
    dev.clear(torch.tensor([False, True]))
    assert torch.isnan(dev.map[1]).all() and torch.isfinite(dev.map[0]).any()
    dev.clear()
    assert torch.isnan(dev.map).all()
