"""The elevation map's slope / step / roughness / cost layers as one HIP launch on the MI355X
(include/rover_elevation_traverse.h) against TorchElevationMap.traverse, its CPU specification.

Everything here is BIT-EQUAL on the seven outputs (cost scan, column class, lethal count, slope, step, rough, cost), but that any
NaN equals any NaN in the four float layers (a lethal cell's roughness may be a NaN of arithmetic, whose payload and sign are not
the specification's business): the kernel is comparisons, integer cell arithmetic, integer extrema of key bits and correctly rounded
fp32 operations in the header's order, and numpy does the same, so equality is derived, not measured.  Every launch must leave
`heights` and `origin` as they were, and every output lies in a frame of payload NaNs (bytes: 0xA5) that must survive.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from isaac_rover_orbit_amd import _fused, _lib
from isaac_rover_orbit_amd.cfg import RayCasterCfg, TraverseCfg
from test_gpu_elevation_fill import GAP_BITS, _bits, _load, _near, _origins, _pair, _poses, _random_maps

pytestmark = pytest.mark.gpu

NAMES = ("cost scan", "column class", "lethal count", "slope", "step", "rough", "cost")
GUARD = 64
# thresholds a random map of unit normal heights meets on both sides
LOOSE = dict(slope_crit=30.0, step_crit=5.0, rough_crit=4.0, w_slope=0.3, w_step=0.45, w_rough=0.25, unknown_cost=-7.5)


def _framed(count, dtype):
    """(the whole buffer, its middle `count` elements): GUARD elements of filler on either side."""
    if dtype == torch.float32:
        whole = torch.full((count + 2 * GUARD,), GAP_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    else:
        whole = torch.full((count + 2 * GUARD,), 0xA5 if dtype == torch.uint8 else -5, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + count]


def _intact(whole, count):
    raw = whole.view(torch.int32) if whole.dtype == torch.float32 else whole
    fill = GAP_BITS if whole.dtype == torch.float32 else (0xA5 if whole.dtype == torch.uint8 else -5)
    return bool((raw[:GUARD] == fill).all()) and bool((raw[GUARD + count:] == fill).all())


def _same(got, want, layer):
    got = got.detach().cpu().numpy().reshape(want.shape)
    if not layer:
        return np.array_equal(_bits(got), _bits(want))
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _check(dev, spec, pos, quat, cfg, layout="aos", heights=None, what="", dense=True):
    """One launch into framed buffers against the specification; `heights`: (device tensor, numpy array) or None for the map."""
    n, G, cols = dev.num_envs, dev.grid, dev.columns
    src = dev.map if heights is None else heights[0]
    h0, o0 = src.clone(), dev.origin.clone()
    sizes = [(n * cols, torch.float32), (n * cols, torch.uint8), (n, torch.int32)] + [(n * G * G, torch.float32)] * 4
    bufs = [_framed(k, dt) for k, dt in sizes]
    views = [bufs[0][1].view(n, cols), bufs[1][1].view(n, cols), bufs[2][1]] + [b[1].view(n, G, G) if dense else None for b in bufs[3:]]
    got = dev.traverse(*_poses(pos, quat, layout), heights=None if heights is None else heights[0], scan_out=views[0], class_out=views[1],
                       count_out=views[2], slope_out=views[3], step_out=views[4], rough_out=views[5], cost_out=views[6], cfg=cfg)
    want = spec.traverse(pos, quat, heights=None if heights is None else heights[1], cfg=cfg)
    torch.cuda.synchronize()
    for i, (g, w, (whole, _), (k, _), nm) in enumerate(zip(got, want, bufs, sizes, NAMES)):
        assert _intact(whole, k), f"{what}: the frame of {nm}"
        if g is None:
            assert i >= 3 and not dense and bool((whole.view(torch.int32) == GAP_BITS).all()), f"{what}: {nm} written"
        else:
            assert _same(g, w, layer=i >= 3), f"{what}: {nm}"
    assert torch.equal(src.view(torch.int32), h0.view(torch.int32)) and torch.equal(dev.origin, o0), f"{what}: heights or origin written"
    return got, want


@pytest.mark.parametrize("G", [8, 16, 32, 64, 128])
def test_random_maps_at_every_kind_of_grid(G):
    """n = 3; 5 %, 50 % and 100 % known with +-0, denormals, +-3e38 and +-inf among the heights; r = 1 and 4; min_support 1 and the
    full neighbourhood; with the four window outputs (every cell gets a verdict) and without (only the cells under the scan's
    columns do).  G = 8 and 16 have fewer cells than threads, 32 two cells per thread, 64 one strip of 8, 128 four strips of 8."""
    n = 3
    dev, spec = _pair(n, G)
    rng = np.random.default_rng(G)
    classes = set()
    for known in (0.05, 0.5, 1.0):
        _load(dev, spec, _random_maps(rng, n, G, known), _origins(n, G))
        pos, quat = _near(spec)
        for r in (1, 4):
            for support in (1, (2 * r + 1) ** 2):
                cfg = TraverseCfg(radius=r, min_support=support, **LOOSE)
                for dense in (True, False):
                    _, want = _check(dev, spec, pos, quat, cfg, dense=dense, what=f"{known} known, r {r}, support {support}, dense {dense}")
                classes |= set(np.unique(want[1]))
                assert known < 1.0 or support > 1 or (want[1] > 0).sum() > 0
    assert classes == {0, 1, 2}


@pytest.mark.parametrize("word", range(7))
def test_a_bad_pose_word_gives_an_unknown_row_and_written_windows(word):
    """NaN (env 1) and inf (env 2) in each of the seven pose floats in turn, in both pose layouts: class 0, count 0, the row
    unknown_cost; the window outputs are written all the same, and env 0 is served as usual."""
    n, G = 3, 16
    dev, spec = _pair(n, G)
    _load(dev, spec, _random_maps(np.random.default_rng(3), n, G, 0.6), _origins(n, G))
    pos, quat = _near(spec)
    pose = np.concatenate([pos, quat], 1)
    pose[1, word], pose[2, word] = np.nan, -np.inf if word % 2 else np.inf
    cfg = TraverseCfg(radius=2, **LOOSE)
    for layout in ("aos", "soa"):
        for dense in (True, False):
            got, want = _check(dev, spec, pose[:, :3], pose[:, 3:], cfg, layout=layout, dense=dense, what=f"{layout}, dense {dense}")
        assert (want[0][1:] == -7.5).all() and not want[1][1:].any() and not want[2][1:].any() and (want[1][0] > 0).any()
        assert (~np.isnan(want[6][1:])).sum() > 100


def test_a_pose_far_from_the_window():
    """10 m from the origin with a 4 m window: every column lies outside, the rows are unknown_cost; the windows are written."""
    n, G = 2, 16
    dev, spec = _pair(n, G)
    _load(dev, spec, _random_maps(np.random.default_rng(5), n, G, 0.5), _origins(n, G))
    pos, quat = _near(spec)
    pos[0, 0] += 10.0
    pos[1, 1] -= 10.0
    for dense in (True, False):
        _, want = _check(dev, spec, pos, quat, TraverseCfg(**LOOSE), dense=dense)
    assert (want[0] == -7.5).all() and not want[1].any() and not want[2].any() and (~np.isnan(want[6])).any()


def test_scan_into_the_columns_of_observation_rows():
    """scan_out aimed at columns 4 ... 964 of a (n + 1, 965) buffer (pitch 965, 4 bytes off): the four leading columns and the
    guard row keep their bits."""
    n, G = 3, 32
    dev, spec = _pair(n, G)
    _load(dev, spec, _random_maps(np.random.default_rng(6), n, G, 0.5), _origins(n, G))
    pos, quat = _near(spec)
    cfg = TraverseCfg(radius=2, **LOOSE)
    want = spec.traverse(pos, quat, cfg=cfg)
    for cost_out in (None, True):
        rows = torch.full((n + 1, 965), GAP_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
        got = dev.traverse(*_poses(pos, quat, "aos"), scan_out=rows[:n, 4:], cost_out=cost_out, cfg=cfg)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == rows.data_ptr() + 16 and got[0][1].data_ptr() % 16 == 4      # row 1 starts 4 bytes off
        raw = rows.view(torch.int32)
        assert (raw[:, :4] == GAP_BITS).all() and (raw[n] == GAP_BITS).all()
        assert all(_same(g, w, layer=False) for g, w in zip(got[:3], want[:3])) and (want[1] > 0).any() and (want[1] == 0).any()


def test_a_five_by_three_scanner():
    n, G = 3, 32
    sc = RayCasterCfg(size=(1.0, 0.5), resolution=0.25)
    assert sc.grid == (5, 3)
    dev, spec = _pair(n, G, cell=0.1, scanner=sc)
    _load(dev, spec, _random_maps(np.random.default_rng(8), n, G, 0.7), _origins(n, G))
    pos, quat = _near(spec, shift=(4.3, -2.4))
    for dense in (True, False):
        got, want = _check(dev, spec, pos, quat, TraverseCfg(radius=3, **LOOSE), dense=dense)
    assert got[0].shape == (n, 15) and (want[1] > 0).any()


def test_each_output_null_in_turn_and_no_scan_at_all():
    """Through the library: with one output NULL the others are what they are with all seven; without cost_scan_out the class and
    the count are not written (and the ray tables may be NULL)."""
    n, G = 3, 16
    dev, spec = _pair(n, G)
    _load(dev, spec, _random_maps(np.random.default_rng(7), n, G, 0.6), _origins(n, G))
    pos, quat = _near(spec)
    p, q = _poses(pos, quat, "aos")
    cfg = TraverseCfg(radius=2, **LOOSE)
    want = spec.traverse(pos, quat, cfg=cfg)
    tc = cfg.to_native()
    sizes = [(n * 961, torch.float32), (n * 961, torch.uint8), (n, torch.int32)] + [(n * G * G, torch.float32)] * 4

    def run(skip, rays=True):
        bufs = [_framed(k, dt) for k, dt in sizes]
        ptrs = [None if i in skip else b[1].data_ptr() for i, b in enumerate(bufs)]
        _fused.launch("rover_elevation_traverse", dev.map.device, dev.cfg, tc, p.data_ptr(), q.data_ptr(), p.stride(1), p.stride(0),
                      dev.map.data_ptr(), dev.origin.data_ptr(), dev.ray_x.data_ptr() if rays else None, dev.nx,
                      dev.ray_y.data_ptr() if rays else None, dev.ny, ptrs[0], 961, *ptrs[1:], n)
        torch.cuda.synchronize()
        return bufs

    cases_ = [((), True)] + [((i,), True) for i in range(1, 7)] + [((3, 4, 5), True), ((1, 2, 3, 4, 5, 6), True), ((3, 4, 5, 6), True),
                                                                    ((0,), True), ((0,), False), ((0, 3, 4, 5), False), ((0, 4, 5, 6), False)]
    for skip, rays in cases_:
        bufs = run(skip, rays)
        unwritten = set(skip) | ({1, 2} if 0 in skip else set())               # no scan: no column class, no count
        for i, ((whole, mid), (k, _), w) in enumerate(zip(bufs, sizes, want)):
            assert _intact(whole, k), (skip, NAMES[i])
            if i in unwritten:
                raw = whole.view(torch.int32) if whole.dtype == torch.float32 else whole
                assert bool((raw == raw[0]).all()), (skip, NAMES[i])
            else:
                assert _same(mid, w, layer=i >= 3), (skip, NAMES[i])
    assert np.array_equal(_bits(dev.map), _bits(spec.map))


@pytest.mark.parametrize("G", [16, 64])
def test_the_map_and_the_fills_window_as_heights(G):
    """heights = the map, and heights = the filled_out of a fill launch in front of it on the same stream: both against the
    specification on the same inputs; the fill gives cells a verdict that the map alone denies them."""
    n = 3
    dev, spec = _pair(n, G)
    _load(dev, spec, _random_maps(np.random.default_rng(11), n, G, 0.3), _origins(n, G))
    pos, quat = _near(spec)
    cfg = TraverseCfg(radius=2, min_support=9, **LOOSE)
    _, on_map = _check(dev, spec, pos, quat, cfg)
    filled = dev.fill(*_poses(pos, quat, "aos"), iterations=3, filled_out=True)[3]
    filled_np = spec.fill(pos, quat, iterations=3)[3]
    for dense in (True, False):
        _, on_filled = _check(dev, spec, pos, quat, cfg, heights=(filled, filled_np), dense=dense)
    assert np.array_equal(_bits(filled), _bits(filled_np))
    assert (~np.isnan(on_filled[6])).sum() > (~np.isnan(on_map[6])).sum() > 0 and (on_filled[1] > 0).sum() > (on_map[1] > 0).sum()


def test_two_calls_into_the_same_buffers_leave_no_stale_state():
    """r = 4 with support 1, then r = 1 with the full neighbourhood and other thresholds into the SAME seven buffers, then the
    first again: each call's outputs are its own."""
    n, G = 3, 64
    dev, spec = _pair(n, G)
    _load(dev, spec, _random_maps(np.random.default_rng(12), n, G, 0.5), _origins(n, G))
    pos, quat = _near(spec)
    p, q = _poses(pos, quat, "soa")
    a = TraverseCfg(radius=4, **LOOSE)
    b = TraverseCfg(radius=1, min_support=9, slope_crit=3.0, step_crit=1.0, rough_crit=0.5, w_slope=0.0, w_step=1.0, w_rough=0.0, unknown_cost=2.0)
    outs = None
    results = []
    for cfg in (a, b, a):
        if outs is None:                                   # the first call allocates, the others write into its buffers
            kw = dict(slope_out=True, step_out=True, rough_out=True, cost_out=True)
        else:
            kw = dict(zip(("scan_out", "class_out", "count_out", "slope_out", "step_out", "rough_out", "cost_out"), outs))
        outs = dev.traverse(p, q, cfg=cfg, **kw)
        want = spec.traverse(pos, quat, cfg=cfg)
        torch.cuda.synchronize()
        assert all(_same(g, w, layer=i >= 3) for i, (g, w) in enumerate(zip(outs, want))), cfg.radius
        results.append(want)
    assert not np.array_equal(results[0][1], results[1][1]) and (results[1][0] == 2.0).any() and (results[0][0] == -7.5).any()
    # and the sparse form after the dense one, into the scan buffers alone
    got = dev.traverse(p, q, cfg=b, scan_out=outs[0], class_out=outs[1], count_out=outs[2])
    torch.cuda.synchronize()
    assert all(_same(g, w, layer=False) for g, w in zip(got[:3], results[1][:3])) and got[3] is None and got[6] is None


def test_the_class_refuses_what_it_cannot_pass_on():
    n, G = 2, 16
    dev, spec = _pair(n, G)
    pos, quat = _near(spec)
    p, q = _poses(pos, quat, "aos")
    with pytest.raises(ValueError, match="TraverseCfg"):
        dev.traverse(p, q)                                 # the map cfg has no traverse and none is given
    t = TraverseCfg()
    for bad in (dict(cfg=TraverseCfg(radius=5)), dict(heights=torch.empty(n, G, G)), dict(heights=torch.empty(n, G, G + 1, device="cuda")),
                dict(heights=torch.empty(n, G, G, dtype=torch.float64, device="cuda")), dict(slope_out=torch.empty(n, G, G)),
                dict(cost_out=torch.empty(n, G + 1, G, device="cuda")), dict(class_out=torch.empty(n, 961, device="cuda")),
                dict(count_out=torch.empty(n + 1, dtype=torch.int32, device="cuda")), dict(scan_out=False),
                dict(scan_out=False, cost_out=True, class_out=torch.empty(n, 961, dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            dev.traverse(p, q, **{"cfg": t, **bad})
    with pytest.raises(_lib.RoverHipError, match="overlap"):
        dev.traverse(p, q, cfg=t, cost_out=dev.map)
    out = dev.traverse(p, q, cfg=t)                        # an empty map: no verdict anywhere; no window outputs unless asked for
    torch.cuda.synchronize()
    assert all(o is None for o in out[3:]) and (out[0] == 1.0).all() and not out[1].any() and not out[2].any()
    out = dev.traverse(p, q, cfg=t, scan_out=False, rough_out=True)
    torch.cuda.synchronize()
    assert out[0] is None and out[1] is None and out[2] is None and torch.isnan(out[5]).all() and out[5].shape == (n, G, G)
    assert C.sizeof(_lib.ElevationTraverseCfg) == _lib.load().rover_elevation_traverse_cfg_bytes()
