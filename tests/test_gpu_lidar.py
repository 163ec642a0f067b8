"""The scanning lidar on the MI355X through its C ABI: table sizes around the wave, the hit points to the bit, the output buffer's
pitch, targeted rays and poses, the yaw frame, the camera as a cross-check and the refusals that need a handle.

The yardstick is ``camera_reference.cast_brute`` (every ray against the mesh's triangle list, float64) on the specification's
float32 ``lidar.world_rays``, under the rule of lidar_cases.check."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from isaac_rover_orbit_amd import lidar
from isaac_rover_orbit_amd.cfg import CameraCfg, LidarCfg
from isaac_rover_orbit_amd.elevation import body_rays
from lidar_cases import DEV, ERR_STATE, Rig, check, flat_terrain, make_env, ptr, quat, random_table, reference, rough

pytestmark = pytest.mark.gpu

RES, MIN_X, MIN_Y = 0.1, -1.0, 2.0
# 48 x 40 cells: the one 64 x 64 block of the pyramid is cut short on both axes
HEIGHT = rough((41, 49), seed=11)
TOP = float(HEIGHT.max())
POSES = ([(0.9, 3.7, TOP + 0.3), (1.6, 4.4, TOP + 0.05), (2.8, 3.1, TOP + 0.6)],
         [quat(0.4, 0.2, -0.15), quat(-2.1, -0.25, 0.1), quat(2.9, 0.1, 0.3)])


@pytest.fixture(scope="module")
def rig():
    r = Rig(3)
    r.bind(HEIGHT, RES, MIN_X, MIN_Y)
    yield r
    r.close()


def _ref(cfg, table, P, Q):
    return reference(cfg, table, HEIGHT, RES, MIN_X, MIN_Y, P, Q)


def _hits_spec(o, d, rng):
    """hits_w of the header from the device's own ranges: float32 product, then float32 sum; +inf on a miss."""
    with np.errstate(all="ignore"):
        h = o[:, None, :] + rng[:, :, None] * d
    return np.where(np.isfinite(rng)[:, :, None], h, np.float32(np.inf)).astype(np.float32)


# ----------------------------------------------------------------------------------------------- (a) table sizes, hits, pitch
@pytest.mark.parametrize("R", [1, 63, 64, 65, 280])
def test_rough_terrain_at_table_sizes_around_the_wave(rig, R):
    """R = 1 ... 65: a tail wave masks its lanes and an env's last wave shares its workgroup with the next env's first; 280 is a
    4 x 70 pattern (five waves per env, so the env boundary falls mid-workgroup).  The ranges under the rule, the hit points bit
    for bit from the device's own ranges -- which pins origins and directions to the bit -- and a pitch of R + 5 whose gap
    stays as it was."""
    if R == 280:
        cfg = LidarCfg(channels=4, vertical_fov_range=(-75.0, -5.0), horizontal_fov_range=(-172.5, 172.5), horizontal_res=5.0,
                       max_distance=math.inf)
        table = lidar.pattern_rays(cfg)
        assert table.shape == (280, 3)
    else:
        cfg, table = LidarCfg(max_distance=50.0), random_table(R, seed=R)
    P, Q = rig.set_poses(*POSES)
    gpu, hits, whole = rig.cast(cfg, table, hits=True, gap=5)
    ref, clear, o, d = _ref(cfg, table, P, Q)
    check(gpu, ref, clear, what=f"R={R}")
    assert np.isfinite(gpu).any()
    assert np.isnan(whole[:, R:]).all() and not np.isnan(gpu).any()                     # the gap is not written
    assert np.array_equal(hits.view(np.uint32), _hits_spec(o, d, gpu).view(np.uint32))
    if R == 280:
        assert np.isinf(gpu).any() and (hits[np.isinf(gpu)] == np.inf).all()            # a miss: three +inf
        again, none, _ = rig.cast(cfg, table, hits=False)                               # hits_w = NULL: the same ranges
        assert none is None and np.array_equal(again.view(np.uint32), gpu.view(np.uint32))


# ------------------------------------------------------------------------------------------------------- (b) targeted rays
AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0.6, 0, 0.8), (0, -0.6, 0.8),
                 (0.6, 0, -0.8), (0, 0.8, -0.6), (-0.8, 0, -0.6), (0, -0.6, -0.8)], np.float32)


def test_axis_aligned_and_upward_rays_and_poses_outside_above_and_below(rig):
    """Exactly axis-aligned entries from level poses (the march's parallel branches), upward rays (misses above the terrain's
    top), a pose outside the terrain looking in, one above its highest point, one under the surface.  Share 0: only a grazing
    ray may differ at all."""
    cfg = LidarCfg(position=(0.0, 0.0, 0.0))
    level = [1.0, 0.0, 0.0, 0.0]
    for name, pos, qs in (("level inside", [(0.95, 3.95, TOP - 0.1), (2.0, 4.0, TOP + 0.2), (3.05, 5.2, 0.05)], [level] * 3),
                          ("outside looking in", [(-1.6, 4.0, TOP + 1.0), (1.5, 6.6, TOP + 1.0), (4.5, 1.7, TOP + 1.2)],
                           [level, quat(-math.pi / 2), quat(2.4, 0.2)]),
                          ("above the top", [(1.0, 4.0, TOP + 3.0), (2.0, 3.0, TOP + 0.001), (0.0, 5.0, TOP + 40.0)],
                           [level, quat(0.3, 0.4), quat(1.0, -0.3, 0.3)]),
                          ("under the surface", [(1.0, 4.0, -3.0), (2.0, 3.0, float(HEIGHT.min()) - 0.01), (2.5, 5.0, -0.6)],
                           [level, quat(0.3, 0.1), quat(1.0, -0.3, 0.3)])):
        P, Q = rig.set_poses(pos, qs)
        gpu, _, _ = rig.cast(cfg, AXES)
        ref, clear, _, _ = _ref(cfg, AXES, P, Q)
        check(gpu, ref, clear, share=0, what=name)
        if name == "level inside":
            assert np.isinf(gpu[1, 5:8]).all() and np.isfinite(gpu[1, 4])               # up: a miss; straight down: a hit
        if name == "above the top":
            assert np.isinf(gpu[0, :4]).all() and np.isinf(gpu[0, 5:8]).all() and np.isfinite(gpu[0, 4])


def test_a_nan_pose_float_gives_that_env_a_row_of_misses(rig):
    cfg, table = LidarCfg(max_distance=50.0), random_table(70, seed=2)
    rig.set_poses(*POSES)
    good, _, _ = rig.cast(cfg, table)
    for word in (0, 2, 3, 6):                                                           # x, z, qw, qz
        pos, qs = np.array(POSES[0], np.float32), np.array(POSES[1], np.float32)
        if word < 3:
            pos[1, word] = np.nan
        else:
            qs[1, word - 3] = np.nan
        rig.set_poses(pos, qs)
        gpu, hits, _ = rig.cast(cfg, table, hits=True)
        assert np.isposinf(gpu[1]).all() and np.isposinf(hits[1]).all(), word
        assert np.array_equal(gpu[[0, 2]].view(np.uint32), good[[0, 2]].view(np.uint32)), word


def test_clips_cut_a_known_hit(rig):
    table = np.array([(0, 0, -1), (0.6, 0, -0.8), (0, -0.6, -0.8)], np.float32)
    P, Q = rig.set_poses(*POSES)
    base = LidarCfg(max_distance=50.0)
    r0, _, _ = rig.cast(base, table)
    assert np.isfinite(r0).all() and r0.min() > 0.3
    lo, hi = float(r0.min()), float(r0.max())
    mid = 0.5 * (lo + hi)
    for cfg in (LidarCfg(near_clip=0.0, max_distance=mid), LidarCfg(near_clip=mid, max_distance=50.0),
                LidarCfg(near_clip=0.9 * lo, max_distance=1.1 * hi), LidarCfg(near_clip=0.0, max_distance=0.9 * lo)):
        gpu, _, _ = rig.cast(cfg, table)
        ref, clear, _, _ = _ref(cfg, table, P, Q)
        check(gpu, ref, clear, share=0, what=f"clips {cfg.near_clip} .. {cfg.max_distance}")
        keep = (r0 >= cfg.near_clip + 1e-3) & (r0 <= cfg.max_distance - 1e-3)
        assert (np.abs(gpu[keep] - r0[keep]) <= 2e-4 * r0[keep] + 2e-4).all()           # a hit inside the clips is the same hit
        assert np.isinf(gpu[r0 > cfg.max_distance + 1e-3]).all()                        # a far clip in front of it: a miss
    assert np.isinf(rig.cast(LidarCfg(max_distance=0.9 * lo), table)[0]).all()


# ------------------------------------------------------------------------------------------------------------ (c) yaw frame
def test_attach_yaw_only_casts_in_the_yaw_frame(rig):
    full = LidarCfg(channels=4, vertical_fov_range=(-75.0, -15.0), horizontal_res=12.0, max_distance=math.inf)
    yaw = LidarCfg(channels=4, vertical_fov_range=(-75.0, -15.0), horizontal_res=12.0, max_distance=math.inf, attach_yaw_only=True)
    table = lidar.pattern_rays(full)
    P, Q = rig.set_poses(*POSES)                                                        # rolled and pitched
    a, _, _ = rig.cast(full, table)
    b, hits, _ = rig.cast(yaw, table, hits=True)
    ref, clear, o, d = _ref(yaw, table, P, Q)
    check(b, ref, clear, what="yaw frame")
    assert np.array_equal(hits.view(np.uint32), _hits_spec(o, d, b).view(np.uint32))
    both = np.isfinite(a) & np.isfinite(b)
    assert both.mean() > 0.4 and (np.abs(a[both] - b[both]) > 1e-3).mean() > 0.9        # not the full-attitude cast


# -------------------------------------------------------------------------------------------------------- (d) camera cross-check
def test_the_camera_table_reproduces_the_camera_render(rig):
    cam = CameraCfg(width=16, height=9)
    cfg = LidarCfg(position=cam.position, near_clip=cam.near_clip, max_distance=cam.far_clip)
    table = body_rays(cam)
    P, Q = rig.set_poses(*POSES)
    gpu, _, _ = rig.cast(cfg, table)
    native = cam.to_native()
    img = torch.full((3, 9, 16), float("nan"), dtype=torch.float32, device=DEV)
    # the workspace the LIDAR prepared serves the camera
    assert rig.lib.rover_camera_render(rig.h, C.byref(native), ptr(rig.ws), ptr(img), rig.stream()) == 0, rig.lib.rover_last_error()
    depth = img.cpu().numpy().reshape(3, -1)
    ref, clear, _, _ = _ref(cfg, table, P, Q)
    check(gpu, ref, clear, what="lidar against the mesh")
    check(gpu, depth.astype(np.float64), clear, what="lidar against the camera")
    assert np.isfinite(depth).mean() > 0.3


# ------------------------------------------------------------------------------------------------------------ (e) refusals
def test_state_refusals_and_one_workspace_for_both_sensors():
    n = 16
    ter = flat_terrain()
    env = make_env(ter, n, camera=CameraCfg(width=16, height=9))
    env.reset()
    lib, h = env._lib, env._h
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    cfg = LidarCfg(channels=2, vertical_fov_range=(-60.0, -30.0), horizontal_res=45.0)
    c = cfg.to_native()
    tab = torch.from_numpy(lidar.pattern_rays(cfg)).to(DEV)
    out = torch.full((n, cfg.rays), float("nan"), device=DEV)
    cam, cws = env.sensors.camera_cfg, ptr(env.sensors.workspace)
    img = torch.empty(n, 9, 16, device=DEV)

    def cast(ws):
        return lib.rover_lidar_cast(h, C.byref(c), ws, ptr(tab), ptr(out), cfg.rays, None, st)

    assert cast(cws) == 0, lib.rover_last_error()                    # the workspace the CAMERA prepared serves the lidar
    torch.cuda.synchronize()
    r = out.cpu().numpy()
    assert np.isfinite(r).all()
    # between rover_step_begin and rover_step_finish
    a, rew = torch.zeros(n, 2, device=DEV), torch.zeros(n, device=DEV)
    flags, force, log = torch.zeros(2, n, dtype=torch.uint8, device=DEV), torch.zeros(39, n, device=DEV), torch.zeros(16, device=DEV)
    obs, mask = torch.zeros(n, env.obs_dim, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    assert lib.rover_step_begin(h, ptr(a), ptr(rew), ptr(flags[0]), ptr(flags[1]), ptr(force), st) == 0
    assert cast(cws) == ERR_STATE and b"between rover_step_begin and rover_step_finish" in lib.rover_last_error()
    assert lib.rover_step_finish(h, ptr(mask), ptr(obs), ptr(force), ptr(log), st) == 0
    assert cast(cws) == 0
    torch.cuda.synchronize()
    r = out.cpu().numpy()                                            # the frame of the state the step left
    assert np.isfinite(r).all()
    # the last prepare wins: a second workspace prepared by the lidar takes the record from the camera's
    nb = int(lib.rover_lidar_workspace_bytes(h))
    assert nb == int(lib.rover_camera_workspace_bytes(h, C.byref(cam))) > 0
    other = torch.zeros((nb + 3) // 4, dtype=torch.float32, device=DEV)
    assert cast(ptr(other)) == ERR_STATE and b"prepare" in lib.rover_last_error()
    assert lib.rover_lidar_prepare(h, ptr(other), nb - 1, st) == 1 and lib.rover_lidar_prepare(h, ptr(other), nb, st) == 0
    assert cast(ptr(other)) == 0 and cast(cws) == ERR_STATE
    assert lib.rover_camera_render(h, C.byref(cam), cws, ptr(img), st) == ERR_STATE
    assert lib.rover_camera_render(h, C.byref(cam), ptr(other), ptr(img), st) == 0
    # a terrain bound again: refused until prepared again
    H, W = env._height_dev.shape
    sp = env._spawns_dev
    assert lib.rover_set_terrain(h, ptr(env._height_dev), ptr(env._obstacle_dev), ptr(env._mask_dev), H, W, float(ter.resolution), float(ter.min_x),
                                 float(ter.min_y), ptr(sp), int(sp.shape[0])) == 0, lib.rover_last_error()
    assert cast(ptr(other)) == ERR_STATE and b"prepare" in lib.rover_last_error()
    assert lib.rover_lidar_prepare(h, ptr(other), nb, st) == 0 and cast(ptr(other)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), r.view(np.uint32))
    env.close()
