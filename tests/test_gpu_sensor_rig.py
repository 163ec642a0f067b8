"""RoverEnv with every sensor on at once on the MI355X: the camera (sensor model, noise, clip; every 3 steps), the lidar (hits,
noise, clip; every 2 steps; 280 rays per env = four full waves and a tail of 24 lanes) and the elevation map behind either of
them.  After reset() and after each of eight steps every published tensor is rebuilt by hand from the public classes on the same
state and counter and compared bit for bit, and the two-set rotation of the buffers is checked on the device."""
import ctypes as C

import numpy as np
import pytest
import torch

from isaac_rover_orbit_amd import _lib, lidar, terrain as T
from isaac_rover_orbit_amd.cfg import CameraCfg, DepthSensorCfg, ElevationMapCfg, LidarCfg, RoverEnvCfg

pytestmark = pytest.mark.gpu

N, SEED = 5, 11
MAP_KEYS = ("elevation_scan", "elevation_known", "elevation_count")


class Unoise:
    def __init__(self, n_min, n_max):
        self.n_min, self.n_max = n_min, n_max


@pytest.fixture(scope="module")
def rough():
    """12.8 m of rough ground; the spawn table's border does not fit, so the spawns are rock-free nodes of the middle 3.2 m."""
    ter = T.make_procedural_terrain((256, 256), seed=7, sigma_z=0.15, n_rocks=3)
    ij = np.argwhere(ter.rock_mask[96:160, 96:160] == 0)[::37][:2 * N] + 96
    assert len(ij) == 2 * N
    ter.spawn_locations = np.stack([ij[:, 1] * T.RESOLUTION + ter.min_x, ij[:, 0] * T.RESOLUTION + ter.min_y,
                                    ter.height[ij[:, 0], ij[:, 1]]], axis=1).astype(np.float32)
    return ter


def all_sensors_cfg(source: str) -> RoverEnvCfg:
    cfg = RoverEnvCfg()
    cfg.scene.num_envs, cfg.sim.device, cfg.terrain.kind, cfg.seed = N, "cuda:0", "custom", SEED
    sensor = DepthSensorCfg(range_min=0.3, range_max=6.0, sigma=(0.002, 0.001, 0.003), p_drop=0.05, p_edge=0.5, disparity_step=0.125)
    cfg.camera = CameraCfg(width=16, height=9, every_n_steps=3, sensor=sensor, noise=Unoise(-0.02, 0.02), clip=(0.0, 6.0))
    cfg.lidar = LidarCfg(channels=4, horizontal_fov_range=(-138.0, 138.0), horizontal_res=4.0, hits=True, every_n_steps=2,
                         noise=Unoise(-0.03, 0.03), clip=(0.0, 8.0))
    cfg.elevation = ElevationMapCfg(source=source)
    return cfg


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


@pytest.mark.parametrize("source", ["camera", "lidar"])
def test_every_published_tensor_is_the_public_classes_on_the_same_state_and_counter(rough, source):
    from isaac_rover_orbit_amd._fused import stream
    from isaac_rover_orbit_amd.depth_sensor import DepthSensor
    from isaac_rover_orbit_amd.elevation import ElevationMap
    from isaac_rover_orbit_amd.envs import RoverEnv
    from isaac_rover_orbit_amd.obs_post import DEPTH_TAG, LIDAR_TAG, ObsPost, image_segments, lidar_segments
    env = RoverEnv(all_sensors_cfg(source), terrain=rough)
    cam, lid, dev = env.cfg.camera, env.cfg.lidar, env.device
    assert lid.azimuths == 70 and lid.rays == 280 and env.sensors.lidar.workspace is env.sensors.workspace
    # the hand-built chain: the C entry point of the render and the public classes, none of them the env's own objects
    sensor = DepthSensor.from_camera(cam, seed=SEED)
    depth_noise = ObsPost(image_segments(cam), cam.height * cam.width, seed=SEED, tag=DEPTH_TAG)
    caster = lidar.Lidar(lid, env, workspace=env.sensors.workspace)
    range_noise = ObsPost(lidar_segments(lid), lid.rays, seed=SEED, tag=LIDAR_TAG)
    if source == "camera":
        second = ElevationMap(env.cfg.elevation, cam, env.cfg.height_scanner, N, dev)
    else:
        second = ElevationMap(env.cfg.elevation, lidar.elevation_geometry(lid), env.cfg.height_scanner, N, dev, rays=lidar.pattern_rays(lid))
    pose = (env.state[_lib.POS:_lib.POS + 3].t(), env.state[_lib.QUAT:_lib.QUAT + 4].t())
    g = torch.Generator(device="cuda").manual_seed(3)
    history = {}                                       # key -> [(tensor, copy)] of every frame published
    restarted = False
    for s in range(9):
        flags = (None, None)
        if s == 0:
            _, extras = env.reset()
        else:
            if s == 5:                                 # env 1 runs out of time in this step: its map starts over
                env.episode_length_buf[1] = env.cfg.max_episode_length - 1
            _, _, term, trunc, extras = env.step(torch.rand(N, 2, device="cuda", generator=g) * 2 - 1)
            flags = (term, trunc)
            restarted |= bool(trunc[1])
        counter = env.call_counter - 1
        assert counter == s and env.common_step_counter == s
        fresh = set(MAP_KEYS)
        frames = {"camera": None, "lidar": None}
        if s % 2 == 0:
            rng = torch.full((N, lid.channels, lid.azimuths), float("nan"), device=dev)
            hits = torch.full((N, lid.rays, 3), float("nan"), device=dev)
            caster.cast(rng, hits)
            range_noise.apply(rng, counter)
            assert _same(extras["lidar_range"], rng) and _same(extras["lidar_hits_w"], hits), s
            assert torch.isfinite(hits).any() and (rng < 8.0).any()
            frames["lidar"] = rng
            fresh |= {"lidar_range", "lidar_hits_w"}
        if s % 3 == 0:
            img = torch.full((N, cam.height, cam.width), float("nan"), device=dev)
            valid = torch.full((N,), -1, dtype=torch.int32, device=dev)
            _lib.check(env._lib.rover_camera_render(env._h, C.byref(env.sensors.camera_cfg), C.c_void_p(env.sensors.workspace.data_ptr()),
                                                    C.c_void_p(img.data_ptr()), stream(dev)), "rover_camera_render")
            sensor.apply(img, counter, valid_out=valid)
            depth_noise.apply(img, counter)
            assert extras["depth"].shape == (N, cam.width, cam.height) and _same(extras["depth"], img.permute(0, 2, 1)), s
            assert _same(extras["depth_valid"], valid) and int(valid.max()) > 0 and int(valid.min()) < cam.height * cam.width
            frames["camera"] = img
            fresh |= {"depth", "depth_valid"}
        if s == 0:
            second.clear()
        want = second.update(frames[source], *pose, reset=flags)
        for key, w in zip(MAP_KEYS, want):
            assert _same(extras[key], w), (s, key)
        assert _same(env.sensors.elevation.map, second.map) and torch.equal(env.sensors.elevation.origin, second.origin), s
        assert extras["rgb"] is None and set(extras) >= fresh | {"rgb", "depth", "depth_valid", "lidar_range", "lidar_hits_w"}
        # two sets in turn: the frame before this one is bit-unchanged, the one before that was overwritten by this one
        for key in ("depth", "depth_valid", "lidar_range", "lidar_hits_w") + MAP_KEYS:
            h = history.setdefault(key, [])
            if key in fresh:
                h.append((extras[key], extras[key].clone()))
                if len(h) >= 2:
                    assert h[-2][0].data_ptr() != h[-1][0].data_ptr() and _same(*h[-2]), (s, key)
                if len(h) >= 3:
                    assert h[-3][0].data_ptr() == h[-1][0].data_ptr(), (s, key)
            else:                                      # no frame: what is published stays, untouched
                assert extras[key].data_ptr() == h[-1][0].data_ptr() and _same(*h[-1]), (s, key)
    assert restarted and int(extras["elevation_count"].max()) > 0
    assert [len(history[k]) for k in ("depth", "lidar_range", "elevation_scan")] == [3, 5, 9]
    assert not _same(history["depth"][0][1], history["depth"][2][1]) and not _same(history["lidar_range"][0][1], history["lidar_range"][2][1])
    env.close()
