"""The depth sensor model as one HIP launch on the MI355X (include/rover_depth_sensor.h, isaac_rover_orbit_amd.depth_sensor) against
TorchDepthSensor, its CPU specification.

Shapes: n in {1, 3, 17} x (H, W) in {(90, 160), (31, 31), (1, 5), (3, 4), (128, 128)}: a partial last quad (961 = 240 * 4 + 1), an
odd width whose row ends fall inside quads, an image without vertical neighbours, and the size limit; (128, 129) is refused.  The
images sit at all four 16-byte phases under a pitch above H * W, in place and out of place; the gap's NaN payloads survive.

  * range, edges (p_edge = 1), dropout (p in {0, 0.3, 1}), quantisation (sigma = 0), fill, valid_out: BIT-EQUAL.  Each is made of
    comparisons, exact uniforms and correctly rounded fp32 operations in a fixed order with contraction off, and numpy float32 does
    the same, so equality is derived, not measured.
  * the Gaussian stage: |fused - spec64| <= s * B + 2 ulp(max(|z|, |s * e|)), B below.
  * the combined case: mask and counts exact, every valid output on the disparity grid, k the spec's off the left-out pixels.
  * the env wiring, determinism, no synchronisation, a side stream.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import depth_sensor_cases as cases
from helpers import small_procedural

pytestmark = pytest.mark.gpu

# B: the bound tests/test_gpu_rollout.py records for this same box_muller device function against float64 (largest
# |eps_kernel - eps_float64| measured over 2**19 draws 5.117e-07, the bound four times that), as tests/test_gpu_obs_post.py uses it.
B = 4.0 * 5.117e-07
NS, SHAPES = (1, 3, 17), ((90, 160), (31, 31), (1, 5), (3, 4), (128, 128))
GAP_BITS = 0x7FC0BEEF                                  # a NaN with a payload: what the pitch's gap and the lead hold


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def _biteq(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _sensor(c, H, W, cls=None):
    from isaac_rover_orbit_amd.depth_sensor import DepthSensor
    return (cls or DepthSensor)(c, H, W, seed=cases.SEED, env_id_offset=cases.OFFSET)


def _spec(c, H, W, x, float64=False):
    from isaac_rover_orbit_amd.depth_sensor import TorchDepthSensor
    spec = TorchDepthSensor(c, H, W, seed=cases.SEED, env_id_offset=cases.OFFSET, float64=float64)
    return spec.stages(x, cases.COUNTER)


def _framed(x, lead, pitch):
    """`x` (n, hw) inside a flat device buffer of NaN payloads: `lead` floats in front, rows `pitch` apart.  Returns (flat, view)."""
    n, hw = x.shape
    flat = torch.full((lead + n * pitch,), GAP_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    view = flat[lead:].view(n, pitch)[:, :hw]
    assert view.data_ptr() % 16 == 4 * lead
    view.copy_(torch.from_numpy(x))
    return flat, view


def _check_frame(flat, lead, n, pitch, hw):
    gap = flat.view(torch.int32)
    assert (gap[:lead] == GAP_BITS).all() and (gap[lead:].view(n, pitch)[:, hw:] == GAP_BITS).all()


def _run_everywhere(c, H, W, x, want, want_valid):
    """The launch at every 16-byte phase, in place and out of place (the output at another phase than the input)."""
    n, hw = x.shape
    pitch = hw + 7 if n > 1 else hw
    sensor = _sensor(c, H, W)
    for lead in (0, 1, 2, 3):
        flat, view = _framed(x, lead, pitch)
        valid = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        assert sensor.apply(view, cases.COUNTER, valid_out=valid) is view
        assert _biteq(view, want), (lead, "in place")
        assert np.array_equal(valid.cpu().numpy(), want_valid)
        _check_frame(flat, lead, n, pitch, hw)
        src_flat, src = _framed(x, lead, pitch)
        dst_flat, dst = _framed(np.zeros_like(x), (lead + 1) % 4, pitch)
        assert sensor.apply(src, cases.COUNTER, out=dst) is dst             # valid_out = NULL
        assert _biteq(dst, want) and _biteq(src, x), (lead, "out of place")
        _check_frame(src_flat, lead, n, pitch, hw)
        _check_frame(dst_flat, (lead + 1) % 4, n, pitch, hw)


@pytest.mark.parametrize("H, W", SHAPES)
@pytest.mark.parametrize("n", NS)
def test_each_stage_alone_is_bit_equal(n, H, W):
    x = cases.blocks(n, H, W)
    for name, c in cases.stage_cfgs().items():
        st = _spec(c, H, W, x)
        assert st["out"].dtype == np.float32
        _run_everywhere(c, H, W, x, st["out"], st["valid"].sum(axis=1).astype(np.int32))
        if name == "drop1":
            assert not st["valid"].any()
        if name == "range" and H * W > 200:
            assert st["valid"].any() and (~st["valid"]).sum() >= 6 * n      # NaN, +-inf, -1, 0 and the denormal; the bounds stay
            assert _biteq(np.where(st["valid"], x, np.float32(0)), st["out"])
    xq = cases.quant_images(n, H, W)
    for name, c in cases.quant_cfgs().items():
        st = _spec(c, H, W, xq)
        _run_everywhere(c, H, W, xq, st["out"], st["valid"].sum(axis=1).astype(np.int32))
        if H * W > 200:                                                     # ties went to even, k < 1 went invalid
            k16 = st["k"][xq == 16.0]
            assert k16.size and (k16 == (2.0 if name == "quant5" else 4.0)).all()
            assert not st["valid"][xq >= 1e6].any() and (st["out"][xq >= 1e6] == -1.0).all() and st["valid"][xq == 0.0].all()


def test_the_size_limit_is_refused_not_launched():
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd.depth_sensor import DepthSensor
    with pytest.raises(ValueError):
        DepthSensor(cases.native(), 128, 129)
    lib = _lib.load()
    buf = torch.zeros(128 * 129, device="cuda")
    c = cases.native(p_drop=1.0, invalid_value=-1.0)
    rc = lib.rover_depth_sensor_apply(C.byref(c), buf.data_ptr(), buf.data_ptr(), 128, 129, 128 * 129, 1, 1, 0, 0, None, None)
    assert rc == 4 and b"16384" in lib.rover_last_error()
    torch.cuda.synchronize()
    assert not buf.any()
    sensor = DepthSensor(cases.native(), 3, 4)
    for bad in (torch.zeros(2, 13, device="cuda"), torch.zeros(2, 24, device="cuda")[:, ::2], torch.zeros(2, 12)):
        with pytest.raises(ValueError):
            sensor.apply(bad, 0)
    good = torch.ones(2, 3, 4, device="cuda")
    with pytest.raises(ValueError):
        sensor.apply(good, 0, out=torch.zeros(3, 12, device="cuda"))
    with pytest.raises(ValueError):
        sensor.apply(good, 0, valid_out=torch.zeros(2, device="cuda"))
    with pytest.raises(_lib.RoverHipError, match="overlap"):
        flat = torch.ones(30, device="cuda")
        sensor.apply(flat[:24].view(2, 12), 0, out=flat[4:28].view(2, 12))
    assert _biteq(sensor.apply(good, 0), np.ones((2, 3, 4), np.float32))    # a contiguous (n, H, W) tensor; the defaults keep 1 m


@pytest.mark.parametrize("H, W", SHAPES)
@pytest.mark.parametrize("n", NS)
def test_gaussian_stage_against_float64(n, H, W):
    """|fused - spec64| <= s * B + 2 ulp(max(|z|, |s * e|)), s the fp32 sigma(z) of step 4, with the other stages off.  Measured on
    the MI355X over the fifteen shapes: the largest |fused - spec64| is 5.302e-07 (n = 17, 128 x 128) and the largest
    max(|fused - spec64| - 2 ulp, 0) / s is 0, against B = 2.047e-06."""
    from isaac_rover_orbit_amd import obs_post
    from isaac_rover_orbit_amd.depth_sensor import NORMAL_TAG
    c = cases.native(sigma=(0.002, 0.001, 0.003))
    x = (0.5 + 7.5 * np.random.default_rng(n * 31 + H * W).random((n, H * W))).astype(np.float32)
    st = _spec(c, H, W, x, float64=True)
    got = _sensor(c, H, W).apply(torch.from_numpy(x.copy()).cuda(), cases.COUNTER).cpu().numpy()
    e = obs_post.normals(cases.SEED, cases.OFFSET + np.arange(n), cases.COUNTER, H * W, NORMAL_TAG)
    s = st["sigma"].astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(x), np.abs(s * e)).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - st["out"])
    excess = np.maximum(err - 2 * ulp, 0.0) / s
    print(f"n={n} {H}x{W}: max |fused - spec64| = {err.max():.3e}, max (err - 2 ulp) / s = {excess.max():.3e} (B = {B:.3e})")
    assert st["valid"].all() and (got != x).mean() > 0.9
    assert (err <= s * B + 2 * ulp).all()


def test_combined_case():
    c, x = cases.combined_cfg(), cases.combined_images()
    n, H, W = cases.COMBINED_N, cases.COMBINED_H, cases.COMBINED_W
    st = _spec(c, H, W, x)
    valid = torch.zeros(n, dtype=torch.int32, device="cuda")
    got = _sensor(c, H, W).apply(torch.from_numpy(x.copy()).cuda(), cases.COUNTER, valid_out=valid).cpu().numpy()
    assert np.array_equal(got != 0.0, st["valid"])                          # invalid_value = 0; a valid output is a positive depth
    assert np.array_equal(valid.cpu().numpy(), st["valid"].sum(axis=1))
    v = st["valid"]
    fb, step = np.float32(c.fb), np.float32(c.disparity_step)
    k = np.rint(np.float64(fb) / got[v].astype(np.float64) / np.float64(step))
    assert _biteq(fb / (k.astype(np.float32) * step), got[v])               # exactly on the disparity grid
    out = cases.left_out(st)
    assert out.sum() <= cases.LEFT_OUT_CAP * v.sum()
    keep = ~out[v]
    print(f"combined: {v.sum()} valid, {out.sum()} left out, k differs on {(k != st['k'][v]).sum()} pixels, "
          f"{(k[keep] != st['k'][v][keep]).sum()} of them kept")
    assert np.array_equal(k[keep], st["k"][v][keep])


def test_deterministic_no_host_synchronisation_and_a_side_stream():
    c, x = cases.combined_cfg(), cases.combined_images()
    sensor = _sensor(c, cases.COMBINED_H, cases.COMBINED_W)
    a, b, d, e = (torch.from_numpy(x.copy()).cuda() for _ in range(4))
    va, vb = (torch.zeros(cases.COMBINED_N, dtype=torch.int32, device="cuda") for _ in range(2))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        sensor.apply(a, cases.COUNTER, valid_out=va)
        sensor.apply(b, cases.COUNTER, valid_out=vb)
        sensor.apply(d, cases.COUNTER + 1)
        with torch.cuda.stream(side):
            sensor.apply(e, cases.COUNTER)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    side.synchronize()
    assert _biteq(a, b) and torch.equal(va, vb) and _biteq(a, e)
    assert (a != d).any()


# ------------------------------------------------------------------------------------------------------------------ the env
@pytest.fixture(scope="module")
def terrain():
    ter = small_procedural()
    ter.make_spawns(2 * 16, seed=41)
    return ter


def _sensor_cfg(**kw):
    from isaac_rover_orbit_amd.cfg import DepthSensorCfg
    base = dict(range_min=0.3, range_max=6.0, p_drop=0.05, p_edge=0.5, disparity_step=0.125)
    base.update(kw)
    return DepthSensorCfg(**base)


def _camera(which, sensor=None, clip=None):
    from isaac_rover_orbit_amd import dagger
    from isaac_rover_orbit_amd.cfg import CameraCfg
    cam = CameraCfg() if which == "reference" else dagger.student_camera_cfg()
    cam.sensor, cam.clip = sensor, clip
    return cam


def _env(terrain, camera, n=16, offset=0):
    from isaac_rover_orbit_amd.cfg import RoverEnvCfg
    from isaac_rover_orbit_amd.envs import RoverEnv
    cfg = RoverEnvCfg(); cfg.scene.num_envs = n; cfg.terrain.kind = "custom"; cfg.seed = 7
    cfg.env_id_offset, cfg.global_num_envs = offset, 16
    cfg.camera = camera
    return RoverEnv(cfg, terrain=terrain)


def _image(env):
    h, w = env.cfg.camera.height, env.cfg.camera.width
    return env.extras["depth"].permute(0, 2, 1).reshape(env.num_envs, h * w).cpu().numpy()


@pytest.mark.parametrize("which", ["reference", "student"])
def test_env_sensor_against_the_specification(terrain, which):
    """sigma = 0, so the image is bit for bit the spec's on the raw twin's render (range, edges, dropout, quantisation, fill), at
    reset and over four steps; two ranks of 8 are the 16; a second run repeats the first; the checkpoint resumes the draws."""
    from isaac_rover_orbit_amd.depth_sensor import TorchDepthSensor, native_cfg
    twin, env, again = _env(terrain, _camera(which)), _env(terrain, _camera(which, _sensor_cfg())), _env(terrain, _camera(which, _sensor_cfg()))
    lo, hi = _env(terrain, _camera(which, _sensor_cfg()), n=8, offset=0), _env(terrain, _camera(which, _sensor_cfg()), n=8, offset=8)
    assert twin.sensors.depth_sensor is None and "depth_valid" not in twin.extras and env.sensors.depth_sensor is not None and env.sensors.depth_post is None
    cam = env.cfg.camera
    spec = TorchDepthSensor(native_cfg(cam), cam.height, cam.width, seed=7)
    g = torch.Generator(device="cuda").manual_seed(2)
    images, sd, a_at = [], None, None
    for k in range(5):
        if k == 0:
            for e in (twin, env, again, lo, hi):
                e.reset()
        else:
            a = torch.rand(16, 2, device="cuda", generator=g) * 2 - 1
            if k == 3:
                sd, a_at = env.state_dict(), a.clone()
            for e in (twin, env, again):
                e.step(a)
            lo.step(a[:8].contiguous()); hi.step(a[8:].contiguous())
        clean = _image(twin)
        assert _biteq(twin.render_depth(), twin.extras["depth"])             # sensor = None: the render, nothing behind it
        c = env.call_counter - 1
        assert c == k
        counts = np.zeros(16, np.int32)
        want = spec.apply(clean.copy(), c, valid_out=counts)
        got = _image(env)
        assert _biteq(got, want)
        dv = env.extras["depth_valid"]
        assert dv.dtype == torch.int32 and dv.shape == (16,) and np.array_equal(dv.cpu().numpy(), counts)
        assert 0 < counts.max() < cam.height * cam.width and (got == 0.0).any()
        assert _biteq(env.render_depth(), env.extras["depth"]) and _biteq(env.render_depth(), env.extras["depth"])
        assert _biteq(_image(again), got) and torch.equal(again.extras["depth_valid"], dv)
        assert _biteq(np.concatenate([_image(lo), _image(hi)]), got)
        assert torch.equal(torch.cat([lo.extras["depth_valid"], hi.extras["depth_valid"]]), dv)
        images.append(got)
    assert not _biteq(images[3], images[4])
    env.load_state_dict(sd)
    env.set_call_counter(sd["call_counter"])
    env.step(a_at)
    assert _biteq(_image(env), images[3])
    env.load_state_dict(sd)                                                  # re-keyed by env.seed()
    env.set_call_counter(sd["call_counter"])
    env.seed(8)
    env.step(a_at)
    assert not _biteq(_image(env), images[3]) and ((_image(env) == 0.0) != (images[3] == 0.0)).any()


def test_env_sensor_runs_ahead_of_the_clip_and_its_noise_is_bounded(terrain):
    """render -> sensor -> clip: a miss is out of range, reads invalid_value = 0 and the clip lifts it to its lower bound (the clip
    first would bring it to 4 m, inside the range).  With sigma > 0 the image obeys the Gaussian stage's bound."""
    from isaac_rover_orbit_amd import obs_post
    from isaac_rover_orbit_amd.depth_sensor import NORMAL_TAG, TorchDepthSensor, native_cfg
    sensor = _sensor_cfg(sigma=(0.002, 0.001, 0.003), disparity_step=0.0)
    twin, env = _env(terrain, _camera("student"), n=4), _env(terrain, _camera("student", sensor, clip=(0.5, 4.0)), n=4)
    assert env.sensors.depth_sensor is not None and env.sensors.depth_post is not None
    cam = env.cfg.camera
    twin.reset(); env.reset()
    clean, got = _image(twin), _image(env)
    st = TorchDepthSensor(native_cfg(cam), cam.height, cam.width, seed=7, float64=True).stages(clean, 0)
    miss = np.isinf(clean)
    assert miss.any() and (got[miss] == 0.5).all() and (got[~st["valid"]] == 0.5).all() and got.min() == 0.5 and got.max() <= 4.0
    assert np.array_equal(env.extras["depth_valid"].cpu().numpy(), st["valid"].sum(axis=1))
    want = np.clip(st["out"], 0.5, 4.0)
    inside = st["valid"] & (st["out"] > 0.5) & (st["out"] < 4.0) & (got > 0.5) & (got < 4.0)
    e = obs_post.normals(7, np.arange(4), 0, cam.height * cam.width, NORMAL_TAG)
    s = st["sigma"].astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(clean), np.abs(s * e)).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)
    assert inside.sum() > 100 and (err[inside] <= (s * B + 2 * ulp)[inside]).all()
    assert (err[st["valid"]] <= (s * B + 2 * ulp)[st["valid"]]).all()       # on a clip bound the error can only shrink
