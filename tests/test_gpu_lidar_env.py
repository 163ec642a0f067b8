"""RoverEnv with ``cfg.lidar`` on the MI355X, on flat ground: the keys and their buffers, the ranges against the plane, off-steps,
noise, an env with the lidar alone and one with both sensors -- and the elevation map built from the lidar: bit-equal to
TorchElevationMap fed the device's own frames, full after one dense frame, within the section-36 bound of the oracle scan,
through in-step and forced resets and a checkpoint."""
import numpy as np
import pytest
import torch

from helpers import flat
from isaac_rover_orbit_amd import _lib, lidar
from isaac_rover_orbit_amd.cfg import CameraCfg, ElevationMapCfg, LidarCfg, RoverEnvCfg
from lidar_cases import dense_cfg

pytestmark = pytest.mark.gpu

N = 8
KEYS = ("elevation_scan", "elevation_known", "elevation_count")


class Unoise:
    def __init__(self, n_min, n_max):
        self.n_min, self.n_max = n_min, n_max


def _env(lidar_cfg, camera=None, elevation=None, n=N):
    from isaac_rover_orbit_amd.envs import RoverEnv
    cfg = RoverEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    cfg.terrain.kind = "custom"
    cfg.lidar, cfg.camera, cfg.elevation = lidar_cfg, camera, elevation
    return RoverEnv(cfg, terrain=flat())


def _zero(env):
    return env.step(torch.zeros(env.num_envs, 2, device=env.device))


def _pose(env):
    S = env.get_state().cpu().numpy()
    return S[:, _lib.POS:_lib.POS + 3].copy(), S[:, _lib.QUAT:_lib.QUAT + 4].copy()


def _i32(a):
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def _extras(env):
    torch.cuda.synchronize()
    return [env.extras[k].cpu().numpy().copy() for k in KEYS]


def _plane(env, frame):
    """The frame against the plane z = 0 from the state's poses: r = o_z / -d_z on the specification's rays where the ray goes
    down and ends inside the terrain and max_distance; the camera tests' bound."""
    cfg = env.cfg.lidar
    o, d = lidar.world_rays(cfg, lidar.pattern_rays(cfg), *_pose(env))
    with np.errstate(all="ignore"):
        want = o[:, None, 2].astype(np.float64) / -d[:, :, 2].astype(np.float64)
    got = frame.reshape(env.num_envs, -1).cpu().numpy().astype(np.float64)
    hit = np.isfinite(got)
    assert hit.mean() > 0.9 and (d[:, :, 2][hit] < 0).all()
    err = np.abs(got - want)[hit]
    assert (err <= 1e-4 * want[hit] + 1e-4).all(), float(err.max())
    return o, d, got


# ---------------------------------------------------------------------------------------------------------------- the sensor
def test_keys_shapes_ranges_and_hits_on_flat_ground():
    env = _env(LidarCfg(hits=True))
    _, extras = env.reset()
    r, h = extras["lidar_range"], extras["lidar_hits_w"]
    assert r.shape == (N, 32, 180) and r.dtype == torch.float32 and h.shape == (N, 5760, 3)
    assert "depth" not in extras and "elevation_scan" not in extras and env.sensors.camera_cfg is None      # a lidar alone works
    torch.cuda.synchronize()
    o, d, got = _plane(env, r)
    with np.errstate(all="ignore"):
        want = o[:, None, :] + got.astype(np.float32)[:, :, None] * d
    want = np.where(np.isfinite(got)[:, :, None], want, np.float32(np.inf)).astype(np.float32)
    assert np.array_equal(h.cpu().numpy().view(np.uint32), want.view(np.uint32))
    _, _, _, _, extras = _zero(env)
    torch.cuda.synchronize()
    _plane(env, extras["lidar_range"])
    env.close()


def test_off_steps_keep_the_frame_and_buffers_rotate():
    env = _env(LidarCfg(every_n_steps=3))
    _, extras = env.reset()
    first = extras["lidar_range"]
    kept = first.clone()
    for step in (1, 2):
        _, _, _, _, extras = _zero(env)
        assert extras["lidar_range"].data_ptr() == first.data_ptr(), step       # no cast: the same frame
    _, _, _, _, extras = _zero(env)                                             # step 3 casts into the other buffer
    third = extras["lidar_range"]
    assert third.data_ptr() != first.data_ptr()
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), kept.view(torch.int32))         # the previous frame stays valid
    assert not torch.equal(third, first)                                        # the rover has settled since the reset
    _plane(env, third)
    for _ in range(3):
        _, _, _, _, extras = _zero(env)
    assert extras["lidar_range"].data_ptr() == first.data_ptr()                 # two buffers, in turn
    env.close()


def test_noise_repeats_on_a_recast_and_moves_with_the_counter():
    from isaac_rover_orbit_amd.obs_post import LIDAR_TAG, TorchObsPost, lidar_segments
    cfg = LidarCfg(channels=8, horizontal_res=10.0, noise=Unoise(-0.05, 0.05), clip=(0.0, 6.0))
    env = _env(cfg)
    clean = _env(LidarCfg(channels=8, horizontal_res=10.0))
    env.reset(), clean.reset()
    _zero(env), _zero(clean)
    torch.cuda.synchronize()
    raw, noisy = clean.extras["lidar_range"].cpu().numpy(), env.extras["lidar_range"].cpu().numpy()
    a, b = env.cast_lidar(), env.cast_lidar()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and a.data_ptr() != b.data_ptr()
    assert np.array_equal(a.cpu().numpy().view(np.uint32), noisy.view(np.uint32))
    # the specification on the clean frame: the same draws, keyed by the counter of the launch that left the state
    counter = env.call_counter - 1
    spec = TorchObsPost(lidar_segments(cfg), cfg.rays, seed=int(env.cfg.seed), tag=LIDAR_TAG)
    want = spec.apply(raw.reshape(N, -1).copy(), counter)
    assert np.array_equal(want.view(np.uint32), noisy.reshape(N, -1).view(np.uint32))
    sel = np.isfinite(raw) & (raw < 5.9)
    moved = np.abs(noisy - raw)[sel]
    assert sel.mean() > 0.5 and moved.max() <= 0.05 + 1e-6 and (moved > 0).mean() > 0.9
    assert noisy.max() <= 6.0                                                   # a miss is clipped to the upper bound
    env.set_call_counter(env.call_counter + 1)                                  # the same state under another counter
    c = env.cast_lidar().cpu().numpy()
    inside = (c < 6.0) & (noisy < 6.0)
    assert inside.mean() > 0.5 and (c[inside] != noisy[inside]).mean() > 0.99
    env.close(), clean.close()


def test_no_lidar_adds_nothing_and_both_sensors_share_one_pyramid():
    env = _env(None, camera=CameraCfg(width=16, height=9))
    _, extras = env.reset()
    assert env.sensors.lidar is None and not any(k.startswith("lidar") for k in extras)
    with pytest.raises(RuntimeError):
        env.cast_lidar()
    depth_alone = extras["depth"].clone()
    env.close()
    env = _env(LidarCfg(), camera=CameraCfg(width=16, height=9), elevation=ElevationMapCfg())
    _, extras = env.reset()
    assert env.sensors.lidar.workspace is env.sensors.workspace                               # one prepared workspace serves both
    assert extras["lidar_range"].shape == (N, 32, 180) and extras["depth"].shape == (N, 16, 9)
    assert "lidar_hits_w" not in extras
    torch.cuda.synchronize()
    assert torch.equal(extras["depth"], depth_alone)      # the camera's path is untouched
    _plane(env, extras["lidar_range"])
    assert env.sensors.elevation.pixels == 16 * 9                                      # source = "camera": the map hangs behind the camera
    _zero(env)
    env.close()


# ------------------------------------------------------------------------------------------------------- the map from the lidar
M = 4


def _map_env(lidar_cfg=None, **kw):
    return _env(lidar_cfg or dense_cfg(), elevation=ElevationMapCfg(source="lidar"), n=M, **kw)


def _spec(env):
    from isaac_rover_orbit_amd.elevation import TorchElevationMap
    return TorchElevationMap(env.cfg.elevation, lidar.elevation_geometry(env.cfg.lidar), env.cfg.height_scanner, M,
                             rays=lidar.pattern_rays(env.cfg.lidar))


def _draws(env, rows):
    tries = env._native_cfg.max_target_tries
    rng = np.random.default_rng(3)
    return (np.asarray(rows, np.int32), rng.random(M).astype(np.float32), rng.random((M, tries)).astype(np.float32),
            rng.random(M).astype(np.float32))


def test_one_dense_frame_fills_the_scan_and_reads_what_the_oracle_reads():
    """After reset() alone the dense pattern knows at least 955 of the 961 columns, and every known column equals the observation's
    own column within 1e-4 * range_max + 1e-4 m (section 36's bound)."""
    env = _map_env()
    obs, extras = env.reset()
    assert env.sensors.camera_cfg is None and extras["elevation_scan"].shape == (M, 961)
    scan, known, count = _extras(env)
    print("known columns per env after one dense frame:", count.tolist())
    assert (count >= 955).all() and np.array_equal(count, known.sum(1).astype(np.int32))
    for _ in range(3):
        obs, _, _, _, extras = _zero(env)
    scan, known, count = _extras(env)
    k = known.astype(bool)
    oracle = obs["policy"][:, 4:].cpu().numpy()
    bound = 1e-4 * env.cfg.elevation.range_max + 1e-4
    err = np.abs(scan.astype(np.float64) - oracle.astype(np.float64))[k].max()
    print(f"known columns per env {count.tolist()}, largest |map scan - oracle scan| {err:.3e} m (bound {bound:.1e})")
    assert err <= bound and (count >= 955).all() and (scan[~k] == 0.0).all()
    env.close()


def test_every_step_is_the_spec_on_the_env_s_own_frames():
    """reset() and four steps with every_n_steps = 2: map, origin, scan, known and count are TorchElevationMap's on
    extras["lidar_range"] (None on a step without a cast) and the state's poses, bit for bit, the in-step reset flags included."""
    env = _map_env(dense_cfg(every_n_steps=2))
    spec = _spec(env)
    env.reset()
    restarted = False
    for s in range(5):
        flags = (None, None)
        if s == 3:                                                              # env 1 runs out of time in this step
            env.episode_length_buf[1] = env.cfg.max_episode_length - 1
        if s:
            _, _, term, trunc, _ = _zero(env)
            flags = (term.cpu().numpy(), trunc.cpu().numpy())
            restarted |= bool(flags[1][1])
        frame = env.extras["lidar_range"].cpu().numpy() if s % 2 == 0 else None
        want = spec.update(frame, *_pose(env), reset=flags)
        for g, w, key in zip(_extras(env), want, KEYS):
            assert np.array_equal(_i32(g), _i32(w.reshape(g.shape))), (s, key)
        assert np.array_equal(_i32(env.sensors.elevation.map.cpu().numpy()), _i32(spec.map)), s
        assert np.array_equal(env.sensors.elevation.origin.cpu().numpy(), spec.origin), s
    assert restarted                                                            # an in-step reset started env 1's map over
    env.close()


def test_resets_start_a_map_over_and_a_checkpoint_round_trips():
    """reset_with_draws of env 2: its map is the spec's for ONE frame at its new pose, the others' are those of an uninterrupted
    run; an in-step reset flag does the same through rover_elevation_step's reset argument (pinned bit for bit above); then
    state_dict() -> a fresh env -> load_state_dict() -> one step: identical extras and maps."""
    a, b = _map_env(LidarCfg()), _map_env(LidarCfg())
    for env in (a, b):
        env.reset()
        for _ in range(3):
            _zero(env)
    assert torch.equal(a.sensors.elevation.map.view(torch.int32), b.sensors.elevation.map.view(torch.int32))
    a.reset_with_draws(np.array([0, 0, 1, 0], np.uint8), *_draws(a, [0, 1, 5, 3]))
    pos, quat = _pose(a)
    assert not np.array_equal(pos[2], _pose(b)[0][2])
    spec = _spec(a)
    _, _, want = spec.update(a.extras["lidar_range"].cpu().numpy(), pos, quat)
    scan, known, count = _extras(a)
    assert count[2] == want[2] > 0
    assert np.array_equal(_i32(a.sensors.elevation.map[2].cpu().numpy()), _i32(spec.map[2]))
    others = [0, 1, 3]
    assert torch.equal(a.sensors.elevation.map[others].view(torch.int32), b.sensors.elevation.map[others].view(torch.int32))
    sd = a.state_dict()
    assert {"elevation_map", "elevation_origin"} <= set(sd)
    c = _map_env(LidarCfg())
    c.reset()
    c.load_state_dict(sd)
    _zero(a), _zero(c)
    for x, y in zip(_extras(a), _extras(c)):
        assert np.array_equal(_i32(x), _i32(y))
    assert torch.equal(a.sensors.elevation.map.view(torch.int32), c.sensors.elevation.map.view(torch.int32))
    assert torch.equal(a.sensors.elevation.origin, c.sensors.elevation.origin) and torch.isfinite(a.sensors.elevation.map).sum() > 1000
    a.close(), b.close(), c.close()


def test_the_map_refuses_what_it_cannot_unproject():
    for bad, text in ((LidarCfg(attach_yaw_only=True), "attach_yaw_only"), (LidarCfg(channels=100), "16384")):
        cfg = RoverEnvCfg(lidar=bad, elevation=ElevationMapCfg(source="lidar"))
        with pytest.raises(ValueError, match=text):
            cfg.validate()
        with pytest.raises(ValueError, match=text):
            _map_env(bad)
