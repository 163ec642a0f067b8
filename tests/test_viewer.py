"""rgb_array viewer, CPU side: ViewerCfg and its refusals, the reference cfg's viewer, the float64 reference renderer against
hand-computed scenes, the rover's wheels on the ground, and the minimal registry's RecordVideo."""
import math
import os
import re

import numpy as np
import pytest

import viewer_reference as vr
from isaac_rover_orbit_amd.cfg import AAURoverEnvCfg, RoverEnvCfg, ViewerCfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _defines(path):
    out = {}
    for name, val in re.findall(r"#define\s+(RR_\w+)\s+(.+?)(?:\s*//.*)?$", open(path).read(), flags=re.M):
        nums = [float(x.rstrip("f")) for x in re.findall(r"-?\d+\.?\d*(?:e-?\d+)?f?", val)]
        out[name] = nums if len(nums) > 1 else nums[0]
    return out


def test_reference_restates_the_kernel_constants():
    d = _defines(os.path.join(ROOT, "isaac_rover_orbit_amd", "csrc", "rover_render.hpp"))
    assert d["RR_CHASSIS_CENTER"] == list(vr.CHASSIS_CENTER) and d["RR_CHASSIS_HALF"] == list(vr.CHASSIS_HALF)
    assert (d["RR_WHEEL_HALF_WIDTH"], d["RR_TARGET_RADIUS"], d["RR_TARGET_Z_OFFSET"]) == (vr.WHEEL_HALF_WIDTH, vr.TARGET_RADIUS,
                                                                                          vr.TARGET_Z_OFFSET)
    assert (d["RR_FOCAL_LENGTH"], d["RR_HORIZONTAL_APERTURE"], d["RR_NEAR_CLIP"], d["RR_FAR_CLIP"]) == (
        vr.FOCAL_LENGTH, vr.HORIZONTAL_APERTURE, vr.NEAR_CLIP, vr.FAR_CLIP)
    assert d["RR_LIGHT_POS"] == list(vr.LIGHT_POS) and (d["RR_K_AMBIENT"], d["RR_K_DIFFUSE"]) == (vr.K_AMBIENT, vr.K_DIFFUSE)
    for k in ("ground", "rock", "chassis", "wheel", "target"):
        assert d[f"RR_ALBEDO_{k.upper()}"] == list(vr.ALBEDO[k])
    assert d["RR_SKY_HORIZON"] == list(vr.SKY_HORIZON) and d["RR_SKY_ZENITH"] == list(vr.SKY_ZENITH)
    assert d["RR_ROCK_EPS"] == vr.ROCK_EPS
    assert (d["RR_ID_SKY"], d["RR_ID_GROUND"], d["RR_ID_ROCK"], d["RR_ID_ENV0"], d["RR_IDS_PER_ENV"]) == (0, 1, 2, 3, 8)
    assert abs(vr.WHEEL_RADIUS - 0.10179) < 1e-12      # RV_WHEEL_CONTACT_RADIUS


def test_viewer_cfg_defaults():
    v = ViewerCfg()
    assert (v.eye, v.lookat, v.resolution, v.origin_type, v.env_index) == ((7.5, 7.5, 7.5), (0.0, 0.0, 0.0), (1280, 720), "world", 0)
    assert abs(2 * math.degrees(math.atan(v.horizontal_aperture / (2 * v.focal_length))) - 60.0) < 1e-4
    assert (v.near_clip, v.far_clip, v.draw_targets) == (0.01, 1e6, True)
    assert RoverEnvCfg().viewer == ViewerCfg()
    assert AAURoverEnvCfg().viewer.eye == (-6.0, -6.0, 3.5)          # rover_env_cfg.py:272
    n = v.to_native(4)
    assert (n.width, n.height, n.origin_type, n.draw_targets) == (1280, 720, 0, 1)
    assert list(n.eye) == [7.5, 7.5, 7.5]


@pytest.mark.parametrize("kw", [
    dict(eye=(float("nan"), 0.0, 1.0)), dict(lookat=(0.0, float("inf"), 0.0)), dict(eye=(1.0, 2.0, 3.0), lookat=(1.0, 2.0, 3.0)),
    dict(eye=(1.0, 2.0, 3.0), lookat=(1.0, 2.0, -5.0)), dict(eye=(1.0, 2.0)), dict(resolution=(0, 720)), dict(resolution=(1280, 8193)),
    dict(focal_length=0.0), dict(horizontal_aperture=float("nan")), dict(near_clip=-1.0), dict(near_clip=5.0, far_clip=5.0),
    dict(origin_type="body"), dict(origin_type="env", env_index=4), dict(origin_type="env", env_index=-1),
    # equal as fp32: lookat - eye is vertical once rounded
    dict(eye=(0.1, 0.0, 3.0), lookat=(0.1 + 1e-9, 0.0, 0.0)),
])
def test_viewer_cfg_refusals(kw):
    with pytest.raises(ValueError):
        ViewerCfg(**kw).validate(num_envs=4)


def test_viewer_cfg_accepts_edges():
    ViewerCfg(resolution=(8192, 1), far_clip=float("inf"), origin_type="env", env_index=3).validate(num_envs=4)
    ViewerCfg(origin_type="env", env_index=3).validate()                 # the env count is checked where it is known


def test_reference_viewer_is_carried():
    from isaac_rover_orbit_amd.compat import orbit_shim
    from isaac_rover_orbit_amd.compat.convert import viewer_from_reference
    ref = orbit_shim.ViewerCfg()
    assert tuple(ref.eye) == (7.5, 7.5, 7.5)
    ref.eye = (-6.0, -6.0, 3.5)                                        # what rover_env_cfg.py:272 does in __post_init__
    v = viewer_from_reference(ref)
    assert (v.eye, v.lookat, v.resolution, v.origin_type) == ((-6.0, -6.0, 3.5), (0.0, 0.0, 0.0), (1280, 720), "world")


# ---------------------------------------------------------------------------------------------- the reference renderer
def _state(n=1):
    s = np.zeros((n, 72))
    s[:, vr.QUAT] = 1.0
    s[:, vr.TARGET_W:vr.TARGET_W + 3] = [1000.0, 1000.0, 0.0]          # off-screen
    return s


def _flat(n=64, z=0.0):
    return np.full((n, n), z), np.zeros((n, n))


def _shade(alb, n, X):
    L = np.asarray(vr.LIGHT_POS) - X
    L /= np.linalg.norm(L)
    return np.rint(255 * np.clip(np.asarray(alb) * (vr.K_AMBIENT + vr.K_DIFFUSE * max(0.0, float(np.dot(n, L)))), 0, 1))


def test_flat_plane_colour_is_the_formula():
    h, ob = _flat()
    s = _state()
    s[0, vr.POS:vr.POS + 3] = [-100, -100, 0]
    o = np.array([[1.0, 1.5, 2.0]])
    d = np.array([[0.3, 0.2, -1.0]]) / np.linalg.norm([0.3, 0.2, -1.0])
    rgb, dep, oid, gap, graze = vr.render_rays(o, d, h, ob, 0.05, 0.0, 0.0, s)
    t = 2.0 / -d[0, 2]
    assert oid[0] == vr.ID_GROUND and abs(dep[0] - t) < 1e-9
    assert (rgb[0] == _shade(vr.ALBEDO["ground"], [0, 0, 1], o[0] + t * d[0])).all()
    ob[10:20, 10:30] = 0.2                                             # a rock under the hit point (x 0.5 .. 1.45, y 0.5 .. 0.95)
    o2 = np.array([[1.0, 0.7, 2.0]])
    rgb, dep, oid, _, _ = vr.render_rays(o2, np.array([[0, 0, -1.0]]), h, ob, 0.05, 0.0, 0.0, s)
    assert oid[0] == vr.ID_ROCK and (rgb[0] == _shade(vr.ALBEDO["rock"], [0, 0, 1], [1.0, 0.7, 0])).all()
    # sky: a ray up
    rgb, dep, oid, _, _ = vr.render_rays(o, np.array([[0.0, 0.6, 0.8]]), h, ob, 0.05, 0.0, 0.0, s)
    sky = np.rint(255 * (np.array(vr.SKY_HORIZON) + 0.8 * (np.array(vr.SKY_ZENITH) - vr.SKY_HORIZON)))
    assert oid[0] == vr.ID_SKY and np.isinf(dep[0]) and (rgb[0] == sky).all()


def test_box_seen_face_on():
    h, ob = _flat(z=-5.0)
    s = _state()
    s[0, vr.POS:vr.POS + 3] = [1.6, 1.6, 0.0]
    o = np.array([[1.6 + 3.0, 1.6, 0.06]])                            # in front of the chassis' +x face, at its centre height
    d = np.array([[-1.0, 0.0, 0.0]])
    rgb, dep, oid, _, _ = vr.render_rays(o, d, h, ob, 0.05, 0.0, 0.0, s)
    assert oid[0] == vr.ID_ENV0 and abs(dep[0] - (3.0 - vr.CHASSIS_HALF[0])) < 1e-12
    assert (rgb[0] == _shade(vr.ALBEDO["chassis"], [1, 0, 0], [1.6 + 0.36, 1.6, 0.06])).all()


def test_cylinder_seen_along_its_axis():
    h, ob = _flat(z=-5.0)
    s = _state()
    s[0, vr.POS:vr.POS + 3] = [1.6, 1.6, 0.0]
    _, _, cen, axl = vr.rover_parts(s[0])
    fl = cen[0]
    assert np.allclose(axl[0], [0, 1, 0]) and np.allclose(fl, [1.6 + 0.44, 1.6 + 0.3925, -0.16699])
    o = fl + [0.0, 2.0, 0.03]                                          # on the FL wheel's axis line (+y side), 3 cm off-centre
    rgb, dep, oid, _, _ = vr.render_rays(o[None], np.array([[0.0, -1.0, 0.0]]), h, ob, 0.05, 0.0, 0.0, s)
    assert oid[0] == vr.ID_ENV0 + 1 and abs(dep[0] - (2.0 - vr.WHEEL_HALF_WIDTH)) < 1e-12   # the cap
    assert (rgb[0] == _shade(vr.ALBEDO["wheel"], [0, 1, 0], o + dep[0] * np.array([0, -1.0, 0]))).all()
    # steered by 90 deg the FL wheel's axle is along -x: the same ray now meets the side of the wheel
    s[0, vr.STEER_Q] = math.pi / 2
    _, _, _, axl = vr.rover_parts(s[0])
    assert np.allclose(axl[0], [-1, 0, 0])
    _, dep, oid, _, _ = vr.render_rays(o[None], np.array([[0.0, -1.0, 0.0]]), h, ob, 0.05, 0.0, 0.0, s)
    assert oid[0] == vr.ID_ENV0 + 1 and abs(dep[0] - (2.0 - math.sqrt(vr.WHEEL_RADIUS ** 2 - 0.03 ** 2))) < 1e-12


def test_sphere_target():
    h, ob = _flat(z=-5.0)
    s = _state()
    s[0, vr.POS:vr.POS + 3] = [-50, -50, 0]
    s[0, vr.TARGET_W:vr.TARGET_W + 3] = [2.0, 2.0, 0.0]
    c = np.array([2.0, 2.0, vr.TARGET_Z_OFFSET])
    o = c + [0.0, 0.05, 4.0]
    rgb, dep, oid, _, _ = vr.render_rays(o[None], np.array([[0, 0, -1.0]]), h, ob, 0.05, 0.0, 0.0, s)
    zt = math.sqrt(vr.TARGET_RADIUS ** 2 - 0.05 ** 2)
    assert oid[0] == vr.ID_ENV0 + 7 and abs(dep[0] - (4.0 - zt)) < 1e-12
    n = np.array([0.0, 0.05, zt]) / vr.TARGET_RADIUS
    assert (rgb[0] == _shade(vr.ALBEDO["target"], n, c + [0, 0.05, zt])).all()
    _, _, oid, _, _ = vr.render_rays(o[None], np.array([[0, 0, -1.0]]), h, ob, 0.05, 0.0, 0.0, s, draw_targets=False)
    assert oid[0] == vr.ID_GROUND


def test_tie_goes_to_the_lower_id():
    h, ob = _flat(z=-5.0)
    s = _state(2)
    s[:, vr.POS:vr.POS + 3] = [1.6, 1.6, 0.0]                          # two envs in the same place: every hit is a tie
    o = np.array([[1.6 + 3.0, 1.6, 0.06]])
    _, _, oid, gap, _ = vr.render_rays(o, np.array([[-1.0, 0, 0]]), h, ob, 0.05, 0.0, 0.0, s)
    assert oid[0] == vr.ID_ENV0 and gap[0] == 0.0
    s[0, vr.POS:vr.POS + 3] = [1.6, 1.6, -0.8]                         # env 0 below the ray: env 1's chassis
    _, _, oid, _, _ = vr.render_rays(o, np.array([[-1.0, 0, 0]]), h, ob, 0.05, 0.0, 0.0, s)
    assert oid[0] == vr.ID_ENV0 + vr.IDS_PER_ENV


def test_wheels_rest_on_flat_ground(oracle):
    """A state the oracle env settles on flat ground: the bottom of every wheel the contact solver loads (normal impulse > 0) touches
    z = 0 within 1 cm -- the reference renderer's wheel kinematics agree with the model the physics integrates.  (A wheel may hang
    free.)"""
    import torch
    from oracle_env import OracleRoverEnv
    from isaac_rover_orbit_amd.terrain import make_flat_terrain
    cfg = RoverEnvCfg()
    cfg.scene.num_envs = 4
    cfg.terrain.kind = "custom"
    env = OracleRoverEnv(cfg, terrain=make_flat_terrain((1024, 1024)))
    env.reset()
    for _ in range(60):
        env.step(torch.zeros(4, 2))
    for e in range(4):
        _, R, cen, axl = vr.rover_parts(env.S[e])
        loaded = env.S[e, 65:71] > 0                                    # ROVER_LAMBDA_N, wheel order FL FR CL CR RL RR
        assert loaded.sum() >= 3
        for k in np.nonzero(loaded)[0]:
            down = np.array([0.0, 0.0, -1.0])
            radial = down - np.dot(down, axl[k]) * axl[k]          # the rim point lowest in the world
            bottom = cen[k] + vr.WHEEL_RADIUS * radial / np.linalg.norm(radial)
            assert abs(bottom[2]) < 0.01, (e, k, bottom)


# ---------------------------------------------------------------------------------------------- RecordVideo (no gymnasium)
class _FakeEnv:
    render_mode = "rgb_array"
    num_envs = 3

    def __init__(self):
        self.k = 0
        self.closed = False

    @property
    def unwrapped(self):
        return self

    def _frame(self):
        return np.full((4, 5, 3), self.k % 256, np.uint8)

    def reset(self, **_):
        self.k = 0
        return {"policy": np.zeros(3)}, {}

    def step(self, a):
        self.k += 1
        done = np.array([self.k % 7 == 0, False, False])
        return {"policy": np.zeros(3)}, np.zeros(3), done, np.zeros(3, bool), {}

    def render(self):
        return self._frame()

    def close(self):
        self.closed = True


def test_minimal_record_video(tmp_path):
    from isaac_rover_orbit_amd.compat import _MiniGym
    gym = _MiniGym()
    env = _FakeEnv()
    w = gym.wrappers.RecordVideo(env, video_folder=str(tmp_path), step_trigger=lambda s: s % 20 == 0, video_length=10,
                                 disable_logger=True)
    assert w.num_envs == 3 and w.unwrapped is env and w.render_mode == "rgb_array"
    w.reset()
    for _ in range(45):
        w.step(None)
    w.close()
    assert env.closed
    files = sorted(os.listdir(tmp_path))
    assert files == ["rl-video-step-0.npz", "rl-video-step-20.npz", "rl-video-step-40.npz"]
    f0 = np.load(tmp_path / "rl-video-step-0.npz")["frames"]
    assert f0.shape == (10, 4, 5, 3) and f0.dtype == np.uint8
    assert [int(f[0, 0, 0]) for f in f0] == list(range(10))           # the state at the trigger, then one frame per step
    f2 = np.load(tmp_path / "rl-video-step-40.npz")["frames"]
    assert [int(f[0, 0, 0]) for f in f2] == list(range(40, 46))       # cut short by close(): what was collected
    # episode trigger (env 0's episode ends every 7 steps), whole episodes
    ep = tmp_path / "ep"
    w = gym.wrappers.RecordVideo(_FakeEnv(), video_folder=str(ep), episode_trigger=lambda e: e == 1, name_prefix="v")
    w.reset()
    for _ in range(20):
        w.step(None)
    assert sorted(os.listdir(ep)) == ["v-episode-1.npz"]
    assert [int(f[0, 0, 0]) for f in np.load(ep / "v-episode-1.npz")["frames"]] == list(range(7, 15))


def test_record_video_needs_rgb_array(tmp_path):
    from isaac_rover_orbit_amd.compat import _MiniGym
    env = _FakeEnv()
    env.render_mode = None
    with pytest.raises(ValueError):
        _MiniGym().wrappers.RecordVideo(env, video_folder=str(tmp_path))


def test_the_envs_share_one_viewer_host_path():
    """Both envs take render / render_frame / render_rgb and the viewport switch from envs/_viewer.py, and the lift's C config
    begins with the rover's (lift_viewer_native copies it member by member)."""
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd.envs import _viewer, lift_env, rover_env
    for name in ("render", "render_frame", "render_rgb"):
        shared = getattr(_viewer.ViewerMixin, name)
        assert getattr(rover_env.RoverEnv, name) is shared and getattr(lift_env.FrankaCubeLiftEnv, name) is shared
    assert lift_env.resolve_render_mode is _viewer.resolve_render_mode is rover_env.resolve_render_mode
    base = _lib.ViewerConfig._fields_
    assert _lib.LiftViewerConfig._fields_[:len(base)] == base
