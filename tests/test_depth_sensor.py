"""The depth sensor model's CPU side (include/rover_depth_sensor.h, isaac_rover_orbit_amd.depth_sensor): TorchDepthSensor, the
specification, against a hand-written per-pixel loop on Python integers and math.*; the row-end rule; every refusal of the library
(no GPU needed: the arguments are checked before the device is looked at); the cfg classes; the tags; shards; the kernel's
resources from the code object; the combined case's left-out share."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import depth_sensor_cases as cases
from isaac_rover_orbit_amd import _lib, depth_sensor
from isaac_rover_orbit_amd.depth_sensor import DROPOUT_TAG, NORMAL_TAG, TorchDepthSensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 0xFFFFFFFF


def f32(x: float) -> float:
    """A Python float rounded to fp32.  +, -, *, / of two fp32 values evaluated in double and rounded once more give the correctly
    rounded fp32 result (double carries more than 2 * 24 + 2 bits), so the loop below is fp32 arithmetic."""
    return C.c_float(x).value


def _philox_by_hand(c, k):
    c, k = [int(v) & F for v in c], [int(v) & F for v in k]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & F, (p0 >> 32) ^ c[3] ^ k[1], p0 & F]
        k = [(k[0] + 0x9E3779B9) & F, (k[1] + 0xBB67AE85) & F]
    return c


def _u(w: int) -> float:
    return ((w >> 9) + 0.5) * 2.0 ** -23


def by_hand(c, img, H, W, seed, env_id, counter):
    """One image (list of H * W floats) through the header's six steps, pixel by pixel.  Returns (out, valid, k) lists."""
    key = (seed & F, seed >> 32)
    ctr = (env_id & F, counter & F, counter >> 32)
    inr = lambda v: v >= c.range_min and v <= c.range_max      # noqa: E731  (False for a NaN)
    out, val, ks = [], [], []
    for p in range(H * W):
        i, j = divmod(p, W)
        z, k = img[p], None
        valid = inr(z)
        if valid:
            edge = False
            for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):                # up, down, left, right
                ii, jj = i + di, j + dj
                if not (0 <= ii < H and 0 <= jj < W):
                    continue
                zn = img[ii * W + jj]
                if not inr(zn):
                    edge = edge or c.edge_at_invalid != 0
                else:
                    edge = edge or abs(f32(z - zn)) > f32(c.edge_rel * min(z, zn))
            u = _u(_philox_by_hand((*ctr, DROPOUT_TAG | (p // 4)), key)[p % 4])
            if u < (c.p_edge if edge else c.p_drop):
                valid = False
        if valid:
            w = _philox_by_hand((*ctr, NORMAL_TAG | (p // 4)), key)
            wa, wb = (w[0], w[1]) if p % 4 < 2 else (w[2], w[3])
            rho, ang = math.sqrt(-2.0 * math.log(_u(wa))), 2.0 * math.pi * _u(wb)
            e = f32(rho * (math.cos(ang) if p % 2 == 0 else math.sin(ang)))
            t = f32(z * c.sigma2)
            t = f32(t + c.sigma1)
            t = f32(z * t)
            s = f32(t + c.sigma0)
            z = f32(z + f32(s * e))
            if c.disparity_step > 0.0:
                d = f32(c.fb / z) if z != 0.0 else math.copysign(math.inf, z)
                k = float(round(f32(d * c.inv_step))) if math.isfinite(d) else d    # Python's round: ties to even
                if not k >= 1.0:
                    valid = False
                else:
                    z = f32(c.fb / f32(k * c.disparity_step))
        out.append(z if valid else c.invalid_value)
        val.append(valid)
        ks.append(k)
    return out, val, ks


@pytest.mark.parametrize("H, W", [(3, 4), (31, 31)])
def test_spec_against_a_hand_written_loop(H, W):
    """All stages on.  The normals of both sides are float64 Box-Muller rounded to fp32; libm and numpy may differ in the last
    bit of log / cos / sin, which would move a rounded normal by one fp32 ulp on rare pixels: those are counted, not hidden --
    every pixel must agree to 2 ulp of the larger of |z| and |sigma e|, and at least 99 % bit for bit."""
    n = 2
    c = cases.native(range_min=0.75, range_max=5.5, sigma=(0.001, 0.0005, 0.002), p_drop=0.1, p_edge=0.6, edge_rel=0.1,
                     disparity_step=0.125, fb=2.8010733127593994, inv_step=8.0, invalid_value=-1.0)
    x = cases.blocks(n, H, W)
    spec = TorchDepthSensor(c, H, W, seed=cases.SEED, env_id_offset=cases.OFFSET)
    st = spec.stages(x, cases.COUNTER)
    counts = np.zeros(n, np.int32)
    got = spec.apply(x.copy(), cases.COUNTER, valid_out=counts)
    assert np.array_equal(got.view(np.int32), st["out"].view(np.int32)) and got.dtype == np.float32
    same = total = 0
    for r in range(n):
        out, val, ks = by_hand(c, [float(v) for v in x[r]], H, W, cases.SEED, cases.OFFSET + r, cases.COUNTER)
        assert val == st["valid"][r].tolist()                                  # range, edges and dropout are exact
        assert counts[r] == sum(val)
        for p in range(H * W):
            if not val[p]:
                assert got[r, p] == -1.0
                continue
            total += 1
            same += float(got[r, p]) == out[p]
            if float(got[r, p]) != out[p]:                                      # one disparity step at the most, on a tie
                assert abs(ks[p] - st["k"][r, p]) <= 1.0, (r, p, ks[p], st["k"][r, p])
    assert total > 0.3 * n * H * W and same >= 0.99 * total, (same, total)
    assert not st["valid"].all() and st["edge"].any() and not st["edge"].all()


def test_noise_stage_alone_against_the_loop_and_the_float64_switch():
    """sigma only: fp32 spec vs the loop within one fp32 ulp of the result (a last-bit difference of the float64 normal), and the
    float64 switch agrees with the fp32 evaluation to rounding."""
    H, W, n = 5, 7, 2
    c = cases.native(sigma=(0.002, 0.001, 0.003))
    x = (1.0 + 4.0 * np.random.default_rng(3).random((n, H * W))).astype(np.float32)
    got = TorchDepthSensor(c, H, W, seed=3, env_id_offset=9).apply(x.copy(), 5)
    for r in range(n):
        out, val, _ = by_hand(c, [float(v) for v in x[r]], H, W, 3, 9 + r, 5)
        assert all(val) and np.abs(got[r] - np.array(out, np.float32)).max() <= np.spacing(np.float32(8.0))
    g64 = TorchDepthSensor(c, H, W, seed=3, env_id_offset=9, float64=True).apply(x.copy(), 5)
    assert g64.dtype == np.float64 and np.abs(g64 - got).max() <= 2 * np.spacing(np.float32(8.0)) and (got != x).mean() > 0.9


def test_row_ends_make_no_edge():
    """A step between the last column of row i and column 0 of row i + 1 is no edge: the flat index does not wrap.  A flat image at
    2 m whose row 0 ends 7.5 % below and whose row 1 starts 7.5 % above: each is within edge_rel = 10 % of its true neighbours, the
    two are 16 % apart."""
    H, W = 3, 6
    c = cases.native(p_edge=1.0)
    img = np.full((1, H, W), 2.0, np.float32)
    img[0, 0, W - 1] = np.float32(1.85)
    img[0, 1, 0] = np.float32(2.15)
    st = TorchDepthSensor(c, H, W).stages(img.reshape(1, -1), 0)
    assert abs(2.15 - 1.85) > 0.1 * 1.85 and not st["edge"].any() and st["valid"].all()
    img[0, 0, W - 2] = np.float32(1.5)                   # a true left neighbour that far away does make one
    st = TorchDepthSensor(c, H, W).stages(img.reshape(1, -1), 0)
    assert st["edge"].reshape(H, W)[0, W - 1] and st["edge"].reshape(H, W)[0, W - 2] and not st["edge"].reshape(H, W)[1, 0]
    # width 1: no pixel has a left or right neighbour
    col = np.array([[1.0, 1.01, 3.0, 3.01]], np.float32)
    st = TorchDepthSensor(c, 4, 1).stages(col, 0)
    assert st["edge"].tolist() == [[False, True, True, False]]
    st = TorchDepthSensor(c, 1, 4).stages(col, 0)
    assert st["edge"].tolist() == [[False, True, True, False]]
    st = TorchDepthSensor(c, 2, 2).stages(col, 0)        # rows (1, 1.01) and (3, 3.01): up / down only
    assert st["edge"].all()


def test_every_refusal_through_the_library():
    lib = _lib.load()
    assert lib.rover_depth_sensor_cfg_bytes() == C.sizeof(_lib.DepthSensorCfg) == 52
    buf = np.zeros(256, np.float32)
    base = buf.ctypes.data                               # never read or written: every call below is refused
    nan, inf = math.nan, math.inf

    def call(cfg=None, null_cfg=False, src=base, dst=base, h=3, w=4, pitch=12, n=2, valid=None):
        cfg = cfg if cfg is not None else cases.native()
        rc = lib.rover_depth_sensor_apply(None if null_cfg else C.byref(cfg), src, dst, h, w, pitch, n, 1, 0, 0, valid, None)
        return rc, lib.rover_last_error().decode()

    q = dict(disparity_step=0.125, fb=2.8, inv_step=8.0)
    refusals = [
        (dict(null_cfg=True), "NULL"), (dict(src=None), "NULL"), (dict(dst=None), "NULL"),
        (dict(n=0), "n must"), (dict(n=-2), "n must"),
        (dict(h=0), "height"), (dict(w=0), "height"), (dict(h=-1), "height"), (dict(w=-4), "height"),
        (dict(pitch=11), "pitch"),
        (dict(src=base + 2, dst=base + 2), "aligned"), (dict(dst=base + 513), "aligned"), (dict(valid=base + 1), "aligned"),
        (dict(dst=base + 4), "overlap"), (dict(src=base + 4 * 23), "overlap"), (dict(dst=base + 4 * 12), "overlap"),
        (dict(cfg=cases.native(sigma=(-0.1, 0, 0))), "sigma"), (dict(cfg=cases.native(sigma=(0, nan, 0))), "sigma"),
        (dict(cfg=cases.native(sigma=(0, 0, inf))), "sigma"), (dict(cfg=cases.native(edge_rel=-1.0)), "edge_rel"),
        (dict(cfg=cases.native(edge_rel=inf)), "edge_rel"), (dict(cfg=cases.native(edge_rel=nan)), "edge_rel"),
        (dict(cfg=cases.native(p_drop=-0.01)), "p_drop"), (dict(cfg=cases.native(p_drop=1.01)), "p_drop"),
        (dict(cfg=cases.native(p_drop=nan)), "p_drop"), (dict(cfg=cases.native(p_edge=2.0)), "p_edge"),
        (dict(cfg=cases.native(p_edge=nan)), "p_edge"), (dict(cfg=cases.native(p_edge=-1.0)), "p_edge"),
        (dict(cfg=cases.native(range_min=nan)), "range_min"), (dict(cfg=cases.native(range_min=-0.5)), "range_min"),
        (dict(cfg=cases.native(range_max=nan)), "range_max"), (dict(cfg=cases.native(range_min=2.0, range_max=1.0)), "range_max"),
        (dict(cfg=cases.native(disparity_step=-0.125)), "disparity_step"), (dict(cfg=cases.native(disparity_step=inf)), "disparity_step"),
        (dict(cfg=cases.native(disparity_step=nan)), "disparity_step"),
        (dict(cfg=cases.native(**{**q, "fb": 0.0})), "fb"), (dict(cfg=cases.native(**{**q, "fb": -1.0})), "fb"),
        (dict(cfg=cases.native(**{**q, "fb": inf})), "fb"), (dict(cfg=cases.native(**{**q, "fb": nan})), "fb"),
        (dict(cfg=cases.native(**{**q, "inv_step": 0.0})), "inv_step"), (dict(cfg=cases.native(**{**q, "inv_step": inf})), "inv_step"),
        (dict(cfg=cases.native(**{**q, "inv_step": nan})), "inv_step"), (dict(cfg=cases.native(**{**q, "inv_step": -8.0})), "inv_step"),
        (dict(cfg=cases.native(invalid_value=nan)), "invalid_value"),
    ]
    for kw, text in refusals:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("rover_depth_sensor_apply:") and text in msg, (kw, rc, msg)
    rc, msg = call(h=128, w=129, pitch=128 * 129)                             # above the limit: unsupported, not invalid
    assert rc == 4 and "16384" in msg
    assert not buf.any()
    # on a host without a GPU, what is allowed gets past the argument checks and fails at the device query instead, with nothing
    # written: range_max = +inf, invalid_value = +-inf and 0, src == dst, fb / inv_step unread without a step, disjoint src and dst
    import torch
    allowed = () if torch.cuda.is_available() else (dict(cfg=cases.native(range_max=inf, invalid_value=inf)), dict(cfg=cases.native(invalid_value=-inf)),
               dict(cfg=cases.native(fb=nan, inv_step=-1.0)), dict(dst=base + 4 * 24), dict(cfg=cases.native(**q)),
               dict(h=128, w=128, pitch=16384, n=1, dst=base))
    for kw in allowed:
        rc, msg = call(**kw)
        assert rc != 0 and not msg.startswith("rover_depth_sensor_apply:"), (kw, rc, msg)
    assert not buf.any()
    # the Python classes refuse the shapes before any call
    for h, w in ((0, 4), (4, 0), (128, 129)):
        with pytest.raises(ValueError):
            TorchDepthSensor(cases.native(), h, w)
    with pytest.raises(TypeError):
        TorchDepthSensor(object(), 3, 4)


def test_cfg_classes_check_the_sensor():
    from isaac_rover_orbit_amd.cfg import CameraCfg, DepthSensorCfg, RoverEnvCfg
    d = DepthSensorCfg()
    assert (d.range_min, d.range_max, d.sigma, d.p_drop, d.p_edge, d.edge_rel, d.edge_at_invalid, d.disparity_step, d.baseline,
            d.invalid_value) == (0.0, math.inf, (0.0, 0.0, 0.0), 0.0, 0.0, 0.1, True, 0.0, 0.05, 0.0)
    assert CameraCfg().sensor is None and RoverEnvCfg().camera is None
    cam = CameraCfg(sensor=DepthSensorCfg(range_min=0.3, range_max=8.0, sigma=(0.001, 0.0, 0.002), p_drop=0.01, p_edge=0.5,
                                          disparity_step=0.125))
    cam.validate()
    c = depth_sensor.native_cfg(cam)
    # fb from the HORIZONTAL focal length, formed in double and rounded once; inv_step likewise
    assert c.fb == float(np.float32(160 * 2.12 / 6.055 * 0.05)) and c.inv_step == 8.0 and c.disparity_step == 0.125
    assert (c.range_min, c.range_max, c.edge_at_invalid) == (float(np.float32(0.3)), 8.0, 1)
    assert (c.sigma0, c.sigma1, c.sigma2) == tuple(float(np.float32(v)) for v in (0.001, 0.0, 0.002))
    cam.vertical_aperture = 2.968879962                                       # f_y moves, fb does not
    assert depth_sensor.native_cfg(cam).fb == c.fb
    nan, inf = math.nan, math.inf
    for bad in (dict(range_min=-1.0), dict(range_min=nan), dict(range_max=nan), dict(range_min=3.0, range_max=2.0),
                dict(sigma=(0.0, -1.0, 0.0)), dict(sigma=(inf, 0.0, 0.0)), dict(sigma=(0.0, 0.0)), dict(p_drop=1.5), dict(p_edge=nan),
                dict(edge_rel=-0.1), dict(disparity_step=-1.0), dict(disparity_step=inf), dict(disparity_step=0.1, baseline=0.0),
                dict(disparity_step=0.1, baseline=-0.05), dict(disparity_step=0.1, baseline=inf), dict(invalid_value=nan)):
        with pytest.raises(ValueError):
            CameraCfg(sensor=DepthSensorCfg(**bad)).validate()
    CameraCfg(sensor=DepthSensorCfg(baseline=0.0)).validate()                 # not read without a disparity step
    CameraCfg(sensor=DepthSensorCfg(invalid_value=inf, range_max=inf)).validate()
    CameraCfg(width=128, height=128, sensor=DepthSensorCfg()).validate()
    with pytest.raises(ValueError, match="16384"):
        CameraCfg(width=129, height=128, sensor=DepthSensorCfg()).validate()
    CameraCfg(width=129, height=128).validate()                               # the limit is the sensor's, not the camera's


def test_example_flags_make_the_sensor_for_both_students():
    import importlib.util
    from isaac_rover_orbit_amd import dagger, dagger_conv
    spec = importlib.util.spec_from_file_location("distil_student_example", os.path.join(ROOT, "examples", "11_distil_student.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    ap = ex.build_parser()
    assert ex.sensor_cfg(ap.parse_args(["--eval", "x.pt", "--depth_noise_std", "0.02"])) is None        # the default: no sensor
    s = ex.sensor_cfg(ap.parse_args(["--eval", "x.pt", "--depth_range", "0.3", "8", "--depth_sigma", "0.001", "0", "0.002",
                                     "--depth_dropout", "0.01", "0.4", "--depth_disparity_step", "0.125", "--depth_baseline", "0.06",
                                     "--depth_invalid", "-1"]))
    assert (s.range_min, s.range_max, s.sigma, s.p_drop, s.p_edge, s.disparity_step, s.baseline, s.invalid_value) == \
        (0.3, 8.0, (0.001, 0.0, 0.002), 0.01, 0.4, 0.125, 0.06, -1.0)
    one = ex.sensor_cfg(ap.parse_args(["--eval", "x.pt", "--depth_dropout", "0.1", "0.5"]))             # one flag: the other defaults
    assert (one.p_drop, one.p_edge, one.range_max, one.disparity_step) == (0.1, 0.5, math.inf, 0.0)
    for cam in (dagger.student_camera_cfg(), dagger_conv.student_camera_cfg()):
        cam.sensor = s
        cam.validate()
        assert depth_sensor.native_cfg(cam).fb == float(np.float32(cam.focal_px[0] * 0.06))


def test_tags_shards_and_counters():
    from isaac_rover_orbit_amd import obs_post
    from isaac_rover_orbit_amd.td3_explore import TAGS
    assert NORMAL_TAG == 0x444E0000 and DROPOUT_TAG == 0x44550000 and not (NORMAL_TAG | DROPOUT_TAG) & 0xFFFF
    taken = {v >> 16 for v in TAGS.values()} | {obs_post.ROW_TAG >> 16, obs_post.DEPTH_TAG >> 16}
    assert len(TAGS) >= 9 and NORMAL_TAG >> 16 != DROPOUT_TAG >> 16 and not {NORMAL_TAG >> 16, DROPOUT_TAG >> 16} & taken
    hdr = open(os.path.join(ROOT, "include", "rover_depth_sensor.h")).read()
    assert dict(re.findall(r"#define ROVER_DEPTH_SENSOR_STREAM_(\w+)\s+(0x[0-9A-Fa-f]{8})u", hdr)) == {"NORMAL": "0x444E0000",
                                                                                                       "DROPOUT": "0x44550000"}
    assert re.search(r"#define ROVER_DEPTH_SENSOR_MAX_PIXELS\s+16384\b", hdr) and depth_sensor.MAX_PIXELS == 16384
    # two shards of 2 + 3 images = the 5 images; the counter and the seed move every draw
    H, W, c = 31, 31, cases.combined_cfg()
    x = cases.blocks(5, H, W)
    whole = TorchDepthSensor(c, H, W, seed=7).apply(x.copy(), 11)
    lo = TorchDepthSensor(c, H, W, seed=7, env_id_offset=0).apply(x[:2].copy(), 11)
    hi = TorchDepthSensor(c, H, W, seed=7, env_id_offset=2).apply(x[2:].copy(), 11)
    assert np.array_equal(np.concatenate([lo, hi]).view(np.int32), whole.view(np.int32))
    assert np.array_equal(TorchDepthSensor(c, H, W, seed=7).apply(x.copy(), 11).view(np.int32), whole.view(np.int32))
    for other in (TorchDepthSensor(c, H, W, seed=7).apply(x.copy(), 12), TorchDepthSensor(c, H, W, seed=8).apply(x.copy(), 11)):
        assert ((other != 0) != (whole != 0)).any()                            # another dropout mask
    out = np.empty_like(x)
    res = TorchDepthSensor(c, H, W, seed=7).apply(x, 11, out=out)             # out of place: the input keeps its bits
    assert res is out and np.array_equal(out.view(np.int32), whole.view(np.int32)) and np.array_equal(x.view(np.int32), cases.blocks(5, H, W).view(np.int32))


def test_kernel_uses_no_scratch_and_one_image_of_lds():
    """No private segment; 16388 floats of image + 8 wave counters of LDS, so two workgroups fit a CU's 160 KiB; 512 threads at
    <= 128 VGPRs: four waves per SIMD."""
    from helpers import gfx950_code_objects
    from isaac_rover_orbit_amd import build
    build.build_extension()
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("ROCm llvm tools not installed")
    seen = 0
    for blob in gfx950_code_objects(_lib.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True).stdout
        for entry in re.split(r"\n\s*- \.", notes):
            m = re.search(r"\.name:\s*\S*(depth_sensor_kernel)\S*", entry)
            if not m or ".private_segment_fixed_size" not in entry:
                continue
            seen += 1
            assert re.search(r"\.private_segment_fixed_size:\s*0\b", entry), "depth_sensor_kernel uses scratch memory"
            lds = int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", entry).group(1))
            assert lds == (16384 + 4) * 4 + 8 * 4 and 2 * lds <= 160 * 1024
            assert re.search(r"\.max_flat_workgroup_size:\s*512\b", entry)
            assert int(re.search(r"\.vgpr_count:\s*(\d+)", entry).group(1)) <= 128, "four waves per SIMD need <= 128 VGPRs"
    assert seen == 1


def test_combined_case_leaves_out_at_most_one_percent():
    """The condition on the combined case's INPUT that tests/test_gpu_depth_sensor.py relies on: of the spec's valid pixels, at
    most 1 % have a float64 d * inv_step within 1e-3 of a half-integer (where a last-bit difference of the normal may move k)."""
    c, x = cases.combined_cfg(), cases.combined_images()
    st = TorchDepthSensor(c, cases.COMBINED_H, cases.COMBINED_W, seed=cases.SEED, env_id_offset=cases.OFFSET).stages(x, cases.COUNTER)
    valid, out = st["valid"], cases.left_out(st)
    share = out.sum() / valid.sum()
    print(f"combined case: {valid.sum()} valid of {valid.size} pixels, {out.sum()} left out ({share:.4%}), edges {st['edge'].mean():.3%}")
    assert share <= cases.LEFT_OUT_CAP
    # the case does exercise every stage: in and out of range, edges and flats, dropped and kept, several disparity levels
    assert 0.5 < valid.mean() < 0.95 and 0.01 < st["edge"][st["in_range"]].mean() < 0.2
    assert (st["in_range"] & ~st["kept"]).sum() > 200 and len(np.unique(st["k"][valid])) > 10 and (st["k"][valid] >= 1).all()
    assert (st["noisy"][valid] != x[valid]).mean() > 0.99
