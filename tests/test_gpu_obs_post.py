"""ORBIT's observation post-processing as one HIP launch on the MI355X (include/rover_obs_post.h, isaac_rover_orbit_amd.obs_post)
against TorchObsPost, its CPU specification.

Shapes: n in {1, 3, 17} x width in {13, 965, 14400}: a partial last quad (13 = 3 * 4 + 1, 965 = 241 * 4 + 1), rows at all four
16-byte phases (a 3860-byte pitch), a row count that is a multiple of nothing, and the camera's image width; one case with a pitch
above the width.

  * uniform, constant, clip, scale, untouched columns: BIT-EQUAL.  Each is one correctly rounded fp32 operation in a fixed order
    with contraction off, and numpy float32 does the same, so equality is derived, not measured.
  * gaussian: |fused - spec64| <= std * B + 2 ulp(max(|x + mean|, |std * e|)), B below.
  * special values against the torch expressions on the device; the env and the camera wiring; determinism; no synchronisation.
"""
import numpy as np
import pytest
import torch

from helpers import small_procedural

pytestmark = pytest.mark.gpu

# B: the bound tests/test_gpu_rollout.py records for this same box_muller device function against float64 (its lines 28-33:
# largest |eps_kernel - eps_float64| measured over 2**19 draws 5.117e-07, the bound four times that).  Restated, not re-derived.
EPS_MEASURED_MAX = 5.117e-07
B = 4.0 * EPS_MEASURED_MAX
FLT_MAX = float(np.finfo(np.float32).max)
NS, WIDTHS = (1, 3, 17), (13, 965, 14400)
SEED, OFFSET, COUNTER = (5 << 32) | 77, 4000, (1 << 32) | 9


class Unoise:
    def __init__(self, n_min, n_max):
        self.n_min, self.n_max = n_min, n_max


class Gnoise:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std


class Bias:
    def __init__(self, bias):
        self.bias = bias


def _mixed(width):
    """constant + scale on 0..2, clip + scale on 2, NOTHING on 3, uniform + clip + scale on 4..width"""
    from isaac_rover_orbit_amd.obs_post import segment
    return [segment(4, width, noise=Unoise(-0.02, 0.03), clip=(-0.25, 0.12), scale=2.0),
            segment(0, 2, noise=Bias(0.125), scale=0.5), segment(2, 3, clip=(0.0, 4.0), scale=0.11)]


def _gauss(width):
    from isaac_rover_orbit_amd.obs_post import segment
    return [segment(0, 3, noise=Gnoise(0.5, 1.0)), segment(4, width, noise=Gnoise(0.01, 0.05))]


@pytest.fixture(scope="module")
def inputs():
    """{(n, width): float32 host rows}: 0.2 * normal, with a NaN of a chosen payload in column 3 of every row (no segment there)."""
    out = {}
    for n in NS:
        for w in WIDTHS:
            x = (0.2 * np.random.default_rng(n * 100003 + w).standard_normal((n, w))).astype(np.float32)
            x[:, 3] = np.array([0x7FC01234 + r for r in range(n)], np.uint32).view(np.float32)
            x.setflags(write=False)
            out[n, w] = x
    return out


def _biteq(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n", NS)
def test_uniform_constant_clip_scale_are_bit_equal(inputs, n, width):
    from isaac_rover_orbit_amd.obs_post import ObsPost, TorchObsPost
    x = inputs[n, width]
    want = TorchObsPost(_mixed(width), width, seed=SEED, env_id_offset=OFFSET).apply(x.copy(), COUNTER)
    dev = torch.from_numpy(x.copy()).cuda()
    got = ObsPost(_mixed(width), width, seed=SEED, env_id_offset=OFFSET).apply(dev, COUNTER)
    assert got is dev and _biteq(got, want)                    # int32 compare: column 3 keeps its NaN payloads
    assert not _biteq(got[:, 4:], x[:, 4:])


def test_rows_at_every_alignment_and_a_pitch_above_the_width(inputs):
    """17 rows of 965 inside a (17, 1000) buffer that itself starts 4, 8 and 12 bytes off a 16-byte boundary: the padding and the
    floats in front keep their bits, the rows are the specification's."""
    from isaac_rover_orbit_amd.obs_post import ObsPost, TorchObsPost
    n, width, pitch = 17, 965, 1000
    x = inputs[n, width]
    want = TorchObsPost(_mixed(width), width, seed=SEED, env_id_offset=OFFSET).apply(x.copy(), COUNTER)
    post = ObsPost(_mixed(width), width, seed=SEED, env_id_offset=OFFSET)
    for lead in (0, 1, 2, 3):
        flat = torch.full((lead + n * pitch,), float("nan"), device="cuda")
        buf = flat[lead:].view(n, pitch)
        assert buf.data_ptr() % 16 == 4 * lead
        buf[:, :width] = torch.from_numpy(x.copy()).cuda()
        before = flat.clone()
        post.apply(buf[:, :width], COUNTER)
        assert _biteq(buf[:, :width], want)
        assert _biteq(buf[:, width:], before[lead:].view(n, pitch)[:, width:]) and _biteq(flat[:lead], before[:lead])


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n", NS)
def test_gaussian_against_float64(inputs, n, width):
    """|fused - spec64| <= std * B + 2 ulp(max(|x + mean|, |std * e|)).  Measured on the MI355X over the nine shapes: the largest
    max(|fused - spec64| - 2 ulp, 0) / std is 4.466e-07 (n = 17, width = 14400, std 0.05), against B = 2.047e-06; the largest
    |fused - spec64| itself is 2.267e-07 at std 1 and 5.223e-08 at std 0.05."""
    from isaac_rover_orbit_amd import obs_post
    from isaac_rover_orbit_amd.obs_post import ObsPost, TorchObsPost
    x = inputs[n, width]
    segs = _gauss(width)
    spec = TorchObsPost(segs, width, seed=SEED, env_id_offset=OFFSET).apply64(x, COUNTER)
    got = ObsPost(segs, width, seed=SEED, env_id_offset=OFFSET).apply(torch.from_numpy(x.copy()).cuda(), COUNTER).cpu().numpy()
    assert _biteq(got[:, 3], x[:, 3])
    e = obs_post.normals(SEED, OFFSET + np.arange(n), COUNTER, width, obs_post.ROW_TAG)
    worst = 0.0
    for s in segs:
        sl = slice(s.col_lo, s.col_hi)
        xm, se = np.abs(x[:, sl].astype(np.float64) + s.a), np.abs(s.b * e[:, sl])
        ulp = np.spacing(np.maximum(xm, se).astype(np.float32)).astype(np.float64)
        err = np.abs(got[:, sl].astype(np.float64) - spec[:, sl])
        worst = max(worst, float((np.maximum(err - 2 * ulp, 0.0) / s.b).max()))
        print(f"n={n} width={width} cols [{s.col_lo}, {s.col_hi}): max |fused - spec64| = {err.max():.3e}, std * B = {s.b * B:.3e}, "
              f"max (err - 2 ulp) / std = {(np.maximum(err - 2 * ulp, 0.0) / s.b).max():.3e} (B = {B:.3e})")
        assert (err <= s.b * B + 2 * ulp).all()
    assert worst <= B


def test_special_values_behave_as_the_torch_expressions():
    """NaN, +-inf, -0.0 and FLT_MAX in noisy and clipped columns, against torch on the device fed the specification's uniforms:
    bit for bit.  Gaussian columns: NaN stays NaN, the infinities and FLT_MAX land on the clip bounds."""
    from isaac_rover_orbit_amd import obs_post
    from isaac_rover_orbit_amd.obs_post import ObsPost, segment
    n, width = 3, 13
    specials = [float("nan"), float("inf"), float("-inf"), -0.0, FLT_MAX, -FLT_MAX, 0.0, 1e-30, 3.0e38]
    x = torch.zeros(n, width)
    for r in range(n):
        for c in range(width):
            x[r, c] = specials[(r * width + c) % len(specials)]
    u = torch.from_numpy(obs_post.uniforms(SEED, OFFSET + np.arange(n), COUNTER, width, obs_post.ROW_TAG)).cuda()
    xd = x.cuda()
    for kw in (dict(noise=Unoise(-0.02, 0.03), clip=(-0.25, 0.12), scale=2.0), dict(noise=Unoise(-1.0, 1.0)),
               dict(noise=Unoise(0.0, 0.0), clip=(-1.0, 1.0)), dict(clip=(-0.5, 3.0e38), scale=-3.0), dict(noise=Bias(-0.125), scale=0.5)):
        s = segment(0, width, **kw)
        want = xd.clone()
        if s.noise == obs_post.UNIFORM:
            want = want + u * s.b + s.a
        elif s.noise == obs_post.CONSTANT:
            want = want + s.a
        if s.has_clip:
            want = want.clip(min=s.clip_lo, max=s.clip_hi)
        if s.scale != 1.0:
            want = want * s.scale
        got = ObsPost([s], width, seed=SEED, env_id_offset=OFFSET).apply(xd.clone(), COUNTER)
        assert _biteq(got, want), kw
    got = ObsPost([segment(0, width, noise=Gnoise(0.0, 0.05), clip=(-0.25, 0.5))], width, seed=SEED, env_id_offset=OFFSET).apply(xd.clone(), COUNTER).cpu()
    assert torch.isnan(got[torch.isnan(x)]).all() and not torch.isnan(got[~torch.isnan(x)]).any()
    assert (got[(x == float("inf")) | (x > 1e38)] == 0.5).all() and (got[(x == float("-inf")) | (x < -1e38)] == -0.25).all()
    small = x.abs() < 1e-20
    assert (got[small].abs() <= 0.05 * 6).all() and got[small].std() > 0.0


def test_deterministic_and_no_host_synchronisation(inputs):
    from isaac_rover_orbit_amd.obs_post import ObsPost
    n, width = 17, 965
    post = ObsPost(_mixed(width), width, seed=SEED, env_id_offset=OFFSET)
    a, b, c = (torch.from_numpy(inputs[n, width].copy()).cuda() for _ in range(3))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        post.apply(a, COUNTER)
        post.apply(b, COUNTER)
        post.apply(c, COUNTER + 1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _biteq(a, b)
    assert (a[:, 4:] != c[:, 4:]).any() and _biteq(a[:, :4], c[:, :4])
    with pytest.raises(ValueError):
        post.apply(torch.zeros(n, width + 1, device="cuda"), 0)
    with pytest.raises(ValueError):
        post.apply(torch.zeros(n, 2 * width, device="cuda")[:, ::2], 0)
    with pytest.raises(ValueError):
        post.apply(torch.zeros(n, width), 0)


# ------------------------------------------------------------------------------------------------------------------ the env
@pytest.fixture(scope="module")
def terrain():
    ter = small_procedural()
    ter.make_spawns(2 * 64, seed=41)
    return ter


def _env(terrain, backend, n=64, offset=0, post=True, camera=None):
    from isaac_rover_orbit_amd.cfg import RoverEnvCfg
    from isaac_rover_orbit_amd.envs import RoverEnv
    cfg = RoverEnvCfg(); cfg.scene.num_envs = n; cfg.terrain.kind = "custom"; cfg.seed = 7
    cfg.env_id_offset, cfg.global_num_envs = offset, 64
    if post:       # the table of test_gpu_user_terms.py::test_observation_noise_clip_scale_follow_orbit_order
        hs = cfg.observations["height_scan"]
        hs.noise, hs.clip, hs.scale = Unoise(-0.02, 0.03), (-0.25, 0.12), 2.0
        cfg.observations["distance"].clip = (0.0, 4.0)
        cfg.observation_post_backend = backend
    else:          # the raw twin: the kernels write every term with scale 1, as they do for a term that is finished behind them
        cfg.observations["distance"].scale = 1.0
    cfg.camera = camera
    return RoverEnv(cfg, terrain=terrain)


def test_env_fused_backend_against_the_specification_and_the_torch_backend(terrain):
    from isaac_rover_orbit_amd.obs_post import TorchObsPost, segments
    raw, tor, fus = _env(terrain, None, post=False), _env(terrain, "torch"), _env(terrain, "fused")
    lo, hi = _env(terrain, "fused", n=32, offset=0), _env(terrain, "fused", n=32, offset=32)
    assert fus._obs_fused is not None and tor._obs_fused is None and not raw._obs_post
    assert fus.kernel_names() == raw.kernel_names() == tor.kernel_names()
    spec = TorchObsPost(segments(fus.cfg), 965, seed=7)

    def check(o_raw, o_fus, o_lo, o_hi):
        c = fus.call_counter - 1                                  # the counter the launch that wrote the row ran under
        want = spec.apply(o_raw["policy"].cpu().numpy().copy(), c)
        assert _biteq(o_fus["policy"], want)
        assert _biteq(torch.cat([o_lo["policy"], o_hi["policy"]]), want)        # two ranks of 32 = the 64 envs
        return want

    o_raw, _ = raw.reset(); o_tor, _ = tor.reset(); o_fus, _ = fus.reset(); o_lo, _ = lo.reset(); o_hi, _ = hi.reset()
    first = check(o_raw, o_fus, o_lo, o_hi)
    assert fus.call_counter == 1 and _biteq(o_fus["policy"][:, :2], o_tor["policy"][:, :2])
    g = torch.Generator(device="cuda").manual_seed(2)
    rows, sd, a_next = [], None, None
    for k in range(6):
        a = torch.rand(64, 2, device="cuda", generator=g) * 2 - 1
        if k == 4:
            sd, a_next = fus.state_dict(), a.clone()
        o_raw, r_r, t_r, u_r, _ = raw.step(a)
        o_tor, r_t, t_t, u_t, _ = tor.step(a)
        o_fus, r_f, t_f, u_f, _ = fus.step(a)
        o_lo, *_ = lo.step(a[:32].contiguous()); o_hi, *_ = hi.step(a[32:].contiguous())
        rows.append(check(o_raw, o_fus, o_lo, o_hi))
        T, F = o_tor["policy"], o_fus["policy"]
        assert _biteq(T[:, :2], F[:, :2]) and _biteq(T[:, 3], F[:, 3]) and _biteq(T[:, 2], F[:, 2])   # untouched + the noiseless clip
        assert _biteq(r_t, r_f) and torch.equal(t_t, t_f) and torch.equal(u_t, u_f) and _biteq(r_r, r_f)
        assert float(F[:, 4:].min()) >= -0.5 and float(F[:, 4:].max()) <= 0.24 and torch.isfinite(F).all()
    assert not np.array_equal(rows[0][:, 4:], rows[1][:, 4:]) and not np.array_equal(first, rows[0])
    # the scene facade still reports the hits of the RAW scan
    assert torch.allclose(fus.scene.sensors["height_scanner"].data.ray_hits_w[..., 2], raw.scene.sensors["height_scanner"].data.ray_hits_w[..., 2],
                          atol=1e-6, equal_nan=True)
    # checkpoint: state + call counter restore the noise bit for bit
    fus.load_state_dict(sd)
    fus.set_call_counter(sd["call_counter"])
    o_again, *_ = fus.step(a_next)
    assert _biteq(o_again["policy"], rows[4])
    # re-keyed by env.seed()
    fus.load_state_dict(sd)
    fus.seed(8)
    o_other, *_ = fus.step(a_next)
    assert not _biteq(o_other["policy"][:, 4:], rows[4][:, 4:])


@pytest.mark.parametrize("which", ["reference", "student"])
def test_camera_noise_and_clip(terrain, which):
    from isaac_rover_orbit_amd import dagger, obs_post
    from isaac_rover_orbit_amd.cfg import CameraCfg
    from isaac_rover_orbit_amd.obs_post import TorchObsPost, image_segments

    def cam(noisy):
        c = CameraCfg() if which == "reference" else dagger.student_camera_cfg()
        if noisy:
            c.noise, c.clip = Gnoise(0.0, 0.02), (0.05, 6.0)
        return c

    twin, env = _env(terrain, None, n=4, post=False, camera=cam(False)), _env(terrain, None, n=4, post=False, camera=cam(True))
    assert twin.sensors.depth_post is None and env.sensors.depth_post is not None
    h, w = env.cfg.camera.height, env.cfg.camera.width
    spec = TorchObsPost(image_segments(env.cfg.camera), h * w, seed=7, tag=obs_post.DEPTH_TAG)
    twin.reset(); env.reset()
    a = torch.full((4, 2), 0.5, device="cuda")
    for k in range(2):
        if k:
            twin.step(a); env.step(a)
        clean = twin.extras["depth"].permute(0, 2, 1).reshape(4, h * w).cpu().numpy()
        assert _biteq(twin.render_depth(), twin.extras["depth"])                    # nothing launched behind a noise-free render
        got = env.extras["depth"].permute(0, 2, 1).reshape(4, h * w).cpu().numpy()
        assert _biteq(env.render_depth(), env.extras["depth"])                      # a re-render of the same state repeats its noise
        c = env.call_counter - 1
        assert c == k
        want = spec.apply64(clean, c)
        miss = np.isinf(clean)
        assert miss.any() and (got[miss] == 6.0).all() and np.isfinite(got).all()  # misses sit at clip_hi
        e = obs_post.normals(7, np.arange(4), c, h * w, obs_post.DEPTH_TAG)
        ulp = np.spacing(np.maximum(np.abs(clean[~miss]), np.abs(0.02 * e[~miss])).astype(np.float32)).astype(np.float64)
        err = np.abs(got[~miss].astype(np.float64) - want[~miss])
        print(f"{which} step {k}: max |fused - spec64| = {err.max():.3e}, bound std * B = {np.float32(0.02) * B:.3e} + 2 ulp")
        assert (err <= float(np.float32(0.02)) * B + 2 * ulp).all()
        inside = ~miss & (clean > 0.2) & (clean < 5.8)
        assert inside.any() and np.abs(got[inside] - clean[inside]).max() <= 0.02 * 6 and (got[inside] != clean[inside]).mean() > 0.9
