"""Depth camera on the MI355X: the HIP ray march against closed forms (planes) and against the float64 reference camera
(procedural terrain with rocks), the pose it renders, its layout and cadence, and that turning it on changes nothing else."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from camera_reference import camera_rays, render as ref_render
from isaac_rover_orbit_amd import _lib
from isaac_rover_orbit_amd import terrain as T
from isaac_rover_orbit_amd.cfg import CameraCfg, RoverEnvCfg, TermCfg

pytestmark = pytest.mark.gpu


def _env(terrain, n, camera=None, **cfg_kw):
    from isaac_rover_orbit_amd.envs import RoverEnv
    cfg = RoverEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    cfg.terrain.kind = "custom"
    cfg.camera = camera
    for k, v in cfg_kw.items():
        setattr(cfg, k, v)
    return RoverEnv(cfg, terrain=terrain)


def _plane_terrain(a, b, c, shape=(256, 256), min_x=-2.0, min_y=1.0):
    H, W = shape
    X, Y = np.meshgrid(min_x + T.RESOLUTION * np.arange(W), min_y + T.RESOLUTION * np.arange(H))
    zero = np.zeros(shape, np.uint8)
    ter = T.Terrain(ground=(a * X + b * Y + c).astype(np.float32), obstacle=np.zeros(shape, np.float32), min_x=min_x, min_y=min_y,
                    rock_mask=zero, safe_rock_mask=zero.copy())
    sp = np.zeros((64, 3), np.float32)
    sp[:, 0], sp[:, 1] = min_x + 3.0, min_y + 3.0
    ter.spawn_locations = sp
    return ter


def _quat(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = (math.cos(yaw / 2), math.sin(yaw / 2), math.cos(pitch / 2), math.sin(pitch / 2),
                              math.cos(roll / 2), math.sin(roll / 2))
    return [cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy]


def _set_poses(env, pos, quat):
    S = env.get_state().clone()
    S[:, _lib.POS:_lib.POS + 3] = torch.as_tensor(np.asarray(pos, np.float32))
    S[:, _lib.QUAT:_lib.QUAT + 4] = torch.as_tensor(np.asarray(quat, np.float32))
    env.set_state(S)
    S = env.get_state().cpu().numpy()
    return S[:, _lib.POS:_lib.POS + 3].astype(np.float64), S[:, _lib.QUAT:_lib.QUAT + 4].astype(np.float64)


def _compare_to_reference(gpu, ref, clear, rel=1e-4, abs_=1e-4):
    """(failing pixels, all of them grazing?) under the rule: agree on hit / miss and within rel * d + abs_."""
    g, r = gpu.astype(np.float64), ref
    same = np.isfinite(g) == np.isfinite(r)
    fin = same & np.isfinite(r)
    ok = same.copy()
    ok[fin] = np.abs(g[fin] - r[fin]) <= rel * r[fin] + abs_
    bad = ~ok
    return int(bad.sum()), bool((clear[bad] <= 1e-3).all())


@pytest.mark.parametrize("a,b,c", [(0.0, 0.0, 0.0), (0.0, 0.0, 0.75), (0.12, -0.08, 0.3), (-0.2, 0.1, -0.4)])
def test_planes_match_the_closed_form(a, b, c):
    ter = _plane_terrain(a, b, c)
    H, W = ter.shape
    x0, y0 = ter.min_x, ter.min_y
    x1, y1 = x0 + (W - 1) * ter.resolution, y0 + (H - 1) * ter.resolution
    xy = [(x0 + 6.0, y0 + 6.0, 0.0, 0.0, 0.0), (x0 + 4.0, y0 + 8.0, 2.1, 0.15, -0.1), (x0 + 9.0, y0 + 3.0, -1.3, -0.2, 0.25),
          (x0 + 6.0, y0 + 6.0, 0.8, 0.3, 0.0),
          (x1 - 0.3, y0 + 6.0, 0.0, 0.0, 0.0),       # at the terrain's edge facing out
          (x0 + 0.2, y1 - 0.4, 2.4, 0.05, 0.1)]      # in a corner facing out
    pos = [(x, y, a * x + b * y + c + 0.3) for x, y, *_ in xy]
    quat = [_quat(yaw, pitch, roll) for _, _, yaw, pitch, roll in xy]
    env = _env(ter, len(xy), CameraCfg())
    env.reset()
    P, Q = _set_poses(env, pos, quat)
    dep = env.render_depth().permute(0, 2, 1).cpu().numpy()      # (N, 90, 160)
    cam = env.cfg.camera
    o, d = camera_rays(cam, P, Q)
    for k in range(len(xy)):
        t = (a * o[k, 0] + b * o[k, 1] + c - o[k, 2]) / (d[k, ..., 2] - a * d[k, ..., 0] - b * d[k, ..., 1])
        p = o[k] + t[..., None] * d[k]
        inside = (t >= cam.near_clip) & (p[..., 0] >= x0) & (p[..., 0] <= x1) & (p[..., 1] >= y0) & (p[..., 1] <= y1)
        exp = np.where(inside, t, np.inf)
        edge = (t >= cam.near_clip) & (np.minimum(np.minimum(np.abs(p[..., 0] - x0), np.abs(p[..., 0] - x1)),
                                                  np.minimum(np.abs(p[..., 1] - y0), np.abs(p[..., 1] - y1))) <= 1e-4)
        g = dep[k].astype(np.float64)
        assert ((np.isfinite(g) == np.isfinite(exp)) | edge).all(), f"pose {k}: miss pattern differs"
        both = np.isfinite(g) & np.isfinite(exp)
        err = np.abs(g[both] - exp[both]) - (1e-5 * exp[both] + 1e-5)
        assert both.sum() > 0 and (err <= 0).all(), f"pose {k}: max excess {err.max():.3e}"
        if k >= 4:
            assert (~np.isfinite(g)).any()
    env.close()


@pytest.fixture(scope="module")
def rocky():
    ter = T.make_procedural_terrain((512, 512), seed=21, n_rocks=40)
    ter.make_spawns(2 * 2048, border_offset=2.0)         # the default 20 m border does not fit a 25.6 m map
    return ter


def test_procedural_terrain_matches_the_reference_camera(rocky):
    n = 64
    rng = np.random.default_rng(5)
    H, W = rocky.shape
    res = rocky.resolution
    env = _env(rocky, n, CameraCfg())
    env.reset()
    i = rng.integers(20, H - 20, n)
    j = rng.integers(20, W - 20, n)
    pos = np.stack([rocky.min_x + j * res, rocky.min_y + i * res, rocky.height[i, j] + rng.uniform(0.1, 0.4, n)], 1)
    quat = [_quat(rng.uniform(-math.pi, math.pi), rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25)) for _ in range(n)]
    P, Q = _set_poses(env, pos, quat)
    gpu = env.render_depth().permute(0, 2, 1).cpu().numpy()
    ref, clear = ref_render(env.cfg.camera, rocky.height, res, rocky.min_x, rocky.min_y, P, Q)
    bad, grazing = _compare_to_reference(gpu, ref, clear)
    assert np.isfinite(ref).mean() > 0.5
    assert bad <= 0.0005 * gpu.size, f"{bad} of {gpu.size} pixels disagree"
    assert grazing, "a failing pixel is not a grazing one"
    env.close()


def _user_reward(env):
    return env.scene["robot"].data.root_lin_vel_b[:, 0]


@pytest.mark.parametrize("n,user", [(2048, False), (100, False), (100, True)])
def test_camera_changes_nothing_else(rocky, n, user):
    kw = {}
    if user:
        from isaac_rover_orbit_amd.cfg import _default_rewards
        rw = _default_rewards()
        rw["forward"] = TermCfg(_user_reward, weight=0.5)
        kw["rewards"] = rw
    off = _env(rocky, n, None, **kw)
    on = _env(rocky, n, CameraCfg(), **kw)
    assert off._slow_path == user and on._slow_path == user
    o1, _ = off.reset()
    o2, _ = on.reset()
    assert torch.equal(o1["policy"], o2["policy"])
    g = torch.Generator(device="cuda:0").manual_seed(3)
    for _ in range(50):
        a = torch.rand(n, 2, device="cuda:0", generator=g) * 2 - 1
        r1 = off.step(a)
        r2 = on.step(a)
        assert torch.equal(r1[0]["policy"], r2[0]["policy"])
        for x, y in zip(r1[1:4], r2[1:4]):
            assert torch.equal(x, y)
        l1, l2 = r1[4]["log"], r2[4]["log"]
        assert list(l1.keys()) == list(l2.keys())
        for k in l1.keys():
            assert torch.equal(l1[k], l2[k]), k
    assert "depth" not in off.extras and "depth" in on.extras
    off.close()
    on.close()


def test_step_image_is_the_pose_the_step_left(rocky):
    n = 100
    env = _env(rocky, n, CameraCfg(), episode_length_s=1.0)      # time-outs every 5 steps: resets inside the window
    env.reset()
    g = torch.Generator(device="cuda:0").manual_seed(9)
    resets_checked = 0
    rng = np.random.default_rng(2)
    for s in range(12):
        a = torch.rand(n, 2, device="cuda:0", generator=g) * 2 - 1
        _, _, term, trunc, extras = env.step(a)
        depth = extras["depth"]
        assert torch.equal(depth, env.render_depth())
        reset = torch.nonzero(term | trunc).flatten().cpu().numpy()
        pick = np.unique(np.concatenate([reset[:2], rng.integers(0, n, 2)])).astype(np.int64)
        resets_checked += min(len(reset), 2)
        S = env.get_state().cpu().numpy()[pick]
        ref, clear = ref_render(env.cfg.camera, rocky.height, rocky.resolution, rocky.min_x, rocky.min_y,
                                S[:, _lib.POS:_lib.POS + 3].astype(np.float64), S[:, _lib.QUAT:_lib.QUAT + 4].astype(np.float64))
        gpu = depth[torch.as_tensor(pick, device=depth.device)].permute(0, 2, 1).cpu().numpy()
        bad, grazing = _compare_to_reference(gpu, ref, clear)
        assert bad <= 0.0005 * gpu.size and grazing, f"step {s}: {bad} pixels disagree"
    assert resets_checked > 0
    env.close()


def test_layout_rgb_and_cadence(rocky):
    n = 8
    env = _env(rocky, n, CameraCfg(every_n_steps=3))
    _, extras = env.reset()
    d = extras["depth"]
    assert d.shape == (n, 160, 90) and d.dtype == torch.float32 and d.device.type == "cuda"
    assert d.stride() == (90 * 160, 1, 160) and not d.is_contiguous()
    assert extras["rgb"] is None
    prev = d.clone()
    for s in range(1, 10):
        _, _, _, _, extras = env.step(torch.ones(n, 2, device="cuda:0"))
        cur = extras["depth"]
        if s % 3 == 0:
            assert not torch.equal(cur, prev)                   # the rover moved: a new image
            assert torch.equal(cur, env.render_depth())
            prev = cur.clone()
        else:
            assert torch.equal(cur, prev)                       # untouched on the other steps
    env.close()


@pytest.mark.parametrize("n", [1, 3, 65])
def test_ragged_batches(rocky, n):
    env = _env(rocky, n, CameraCfg())
    _, extras = env.reset()
    d = extras["depth"]
    assert d.shape == (n, 160, 90)
    pick = np.array(sorted({0, n // 2, n - 1}))
    S = env.get_state().cpu().numpy()[pick]
    ref, clear = ref_render(env.cfg.camera, rocky.height, rocky.resolution, rocky.min_x, rocky.min_y,
                            S[:, _lib.POS:_lib.POS + 3].astype(np.float64), S[:, _lib.QUAT:_lib.QUAT + 4].astype(np.float64))
    gpu = d[torch.as_tensor(pick, device=d.device)].permute(0, 2, 1).cpu().numpy()
    bad, grazing = _compare_to_reference(gpu, ref, clear)
    assert bad <= 0.0005 * gpu.size and grazing
    assert np.isfinite(gpu).any()
    env.close()


def test_render_refuses_a_terrain_rebound_without_prepare(rocky):
    env = _env(rocky, 4, CameraCfg())
    env.reset()
    lib, h = env._lib, env._h
    buf = torch.empty(4, 90, 160, device="cuda:0")
    cfg = env.sensors.camera_cfg
    ws = C.c_void_p(env.sensors.workspace.data_ptr())
    assert lib.rover_camera_render(h, C.byref(cfg), ws, C.c_void_p(buf.data_ptr()), None) == 0
    H, W = rocky.shape
    assert lib.rover_set_terrain(h, C.c_void_p(env._height_dev.data_ptr()), C.c_void_p(env._obstacle_dev.data_ptr()),
                                 C.c_void_p(env._mask_dev.data_ptr()), H, W, float(rocky.resolution), float(rocky.min_x),
                                 float(rocky.min_y), C.c_void_p(env._spawns_dev.data_ptr()), int(env._spawns_dev.shape[0])) == 0
    assert lib.rover_camera_render(h, C.byref(cfg), ws, C.c_void_p(buf.data_ptr()), None) == 2      # ROVER_ERR_STATE
    assert b"prepare" in lib.rover_last_error()
    nb = lib.rover_camera_workspace_bytes(h, C.byref(cfg))
    assert lib.rover_camera_prepare(h, C.byref(cfg), ws, nb, None) == 0
    assert lib.rover_camera_render(h, C.byref(cfg), ws, C.c_void_p(buf.data_ptr()), None) == 0
    torch.cuda.synchronize()
    env.close()
