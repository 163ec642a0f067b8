"""RoverEnv with ``cfg.elevation`` on the MI355X: the map behind the camera chain, against the oracle scan on a flat terrain (the one
tolerance test), against TorchElevationMap on the env's own depth images and poses (bit-equal), through in-step and forced resets,
steps without a render, and a checkpoint."""
import numpy as np
import pytest
import torch

import elevation_cases as cases
from helpers import flat
from isaac_rover_orbit_amd import _lib
from isaac_rover_orbit_amd.cfg import CameraCfg, ElevationMapCfg, RoverEnvCfg

pytestmark = pytest.mark.gpu

N = 4
KEYS = ("elevation_scan", "elevation_known", "elevation_count")


def _env(elevation=True, **camera_kw):
    from isaac_rover_orbit_amd.envs import RoverEnv
    cfg = RoverEnvCfg()
    cfg.scene.num_envs = N
    cfg.sim.device = "cuda:0"
    cfg.terrain.kind = "custom"
    cfg.camera = CameraCfg(**camera_kw)
    cfg.elevation = ElevationMapCfg() if elevation else None
    return RoverEnv(cfg, terrain=flat())


def _zero(env):
    return env.step(torch.zeros(N, 2, device=env.device))


def _pose(env):
    S = env.get_state().cpu().numpy()
    return S[:, _lib.POS:_lib.POS + 3].copy(), S[:, _lib.QUAT:_lib.QUAT + 4].copy()


def _spec(env):
    from isaac_rover_orbit_amd.elevation import TorchElevationMap
    return TorchElevationMap(env.cfg.elevation, env.cfg.camera, env.cfg.height_scanner, N)


def _extras(env):
    torch.cuda.synchronize()
    return [env.extras[k].cpu().numpy().copy() for k in KEYS]


def _i32(a):
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def _draws(env, rows):
    tries = env._native_cfg.max_target_tries
    rng = np.random.default_rng(3)
    return (np.asarray(rows, np.int32), rng.random(N).astype(np.float32), rng.random((N, tries)).astype(np.float32),
            rng.random(N).astype(np.float32))


def test_the_map_reads_what_the_oracle_scan_reads_on_flat_ground():
    """After reset() and three zero-action steps every known column equals the observation's own column within 1e-4 * range_max +
    1e-4 m: the camera test's depth bound (tests/test_gpu_camera.py::_compare_to_reference) at the range cap; on a plane the cell
    maximum adds nothing to it.  The 91 corridor columns are known in every env, and the count is the row sum of the known bytes."""
    env = _env()
    obs, extras = env.reset()
    assert all(k in extras for k in KEYS) and extras["elevation_scan"].shape == (N, 961)
    assert extras["elevation_known"].dtype == torch.uint8 and extras["elevation_count"].dtype == torch.int32
    for _ in range(3):
        obs, _, _, _, extras = _zero(env)
    scan, known, count = _extras(env)
    oracle = obs["policy"][:, 4:].cpu().numpy()
    k = known.astype(bool)
    bound = 1e-4 * env.cfg.elevation.range_max + 1e-4
    err = np.abs(scan.astype(np.float64) - oracle.astype(np.float64))[k].max()
    print(f"known columns per env {k.sum(1).tolist()}, largest |map scan - oracle scan| {err:.3e} m (bound {bound:.1e})")
    assert err <= bound
    front, _ = cases.corridor(env.cfg.height_scanner)
    assert front.sum() == 91 and k[:, front].all()
    assert np.array_equal(count, k.sum(1).astype(np.int32)) and (scan[~k] == 0.0).all()
    env.close()


def test_every_step_is_the_spec_on_the_env_s_own_images():
    """reset() and three steps: map, origin, scan, known and count are TorchElevationMap's on extras["depth"] and the state's
    poses, bit for bit, the in-step reset flags included."""
    env = _env()
    spec = _spec(env)
    env.reset()
    for s in range(4):
        flags = (None, None)
        if s:
            _, _, term, trunc, _ = _zero(env)
            flags = (term.cpu().numpy(), trunc.cpu().numpy())
        depth = env.extras["depth"].permute(0, 2, 1).contiguous().cpu().numpy()
        want = spec.update(depth, *_pose(env), reset=flags)
        for g, w, key in zip(_extras(env), want, KEYS):
            assert np.array_equal(_i32(g), _i32(w.reshape(g.shape))), (s, key)
        assert np.array_equal(_i32(env.sensors.elevation.map.cpu().numpy()), _i32(spec.map)), s
        assert np.array_equal(env.sensors.elevation.origin.cpu().numpy(), spec.origin), s
    env.close()


def test_a_forced_reset_starts_one_map_over():
    """reset_with_draws of env 2: its count is the spec's for ONE frame at its new pose; the other envs' maps are those of an
    uninterrupted run, bit for bit, also one step later."""
    a, b = _env(), _env()
    for env in (a, b):
        env.reset()
        for _ in range(3):
            _zero(env)
    assert torch.equal(a.sensors.elevation.map.view(torch.int32), b.sensors.elevation.map.view(torch.int32))
    mask = np.array([0, 0, 1, 0], np.uint8)
    a.reset_with_draws(mask, *_draws(a, [0, 1, 5, 3]))
    pos, quat = _pose(a)
    assert not np.array_equal(pos[2], _pose(b)[0][2]) and np.array_equal(pos[[0, 1, 3]], _pose(b)[0][[0, 1, 3]])
    spec = _spec(a)
    _, _, want = spec.update(a.extras["depth"].permute(0, 2, 1).contiguous().cpu().numpy(), pos, quat)
    scan, known, count = _extras(a)
    assert count[2] == want[2] > 0 and count[2] == known[2].sum()
    assert np.array_equal(_i32(a.sensors.elevation.map[2].cpu().numpy()), _i32(spec.map[2]))
    others = [0, 1, 3]
    assert torch.equal(a.sensors.elevation.map[others].view(torch.int32), b.sensors.elevation.map[others].view(torch.int32))
    assert (count[others] > want[others]).any()                    # they remember more than one frame shows
    _zero(a), _zero(b)
    assert torch.equal(a.sensors.elevation.map[others].view(torch.int32), b.sensors.elevation.map[others].view(torch.int32))
    for x, y in zip(_extras(a), _extras(b)):
        assert np.array_equal(_i32(x[others]), _i32(y[others]))
    a.close(), b.close()


def test_a_step_without_a_render_scrolls_and_scans_only():
    """every_n_steps = 2: the step that renders nothing equals the spec's depth = None update."""
    env = _env(every_n_steps=2)
    spec = _spec(env)
    env.reset()
    _zero(env), _zero(env)                                         # steps 1 (no render) and 2 (render)
    spec.load_state_dict(env.sensors.elevation.state_dict())
    depth_before = env.extras["depth"]
    _, _, term, trunc, extras = _zero(env)                         # step 3: no render
    assert extras["depth"] is depth_before or extras["depth"].data_ptr() == depth_before.data_ptr()
    want = spec.update(None, *_pose(env), reset=(term.cpu().numpy(), trunc.cpu().numpy()))
    for g, w, key in zip(_extras(env), want, KEYS):
        assert np.array_equal(_i32(g), _i32(w.reshape(g.shape))), key
    assert np.array_equal(_i32(env.sensors.elevation.map.cpu().numpy()), _i32(spec.map)) and want[2].min() >= 91
    env.close()


def test_without_a_map_nothing_changes():
    env = _env(elevation=False)
    _, extras = env.reset()
    _, _, _, _, extras = _zero(env)
    assert not any(k in extras for k in KEYS) and "depth" in extras and env.sensors.elevation is None
    assert set(env.state_dict()) == {"state", "obs", "log", "num_envs", "common_step_counter", "call_counter", "seed_lo", "seed_hi"}
    env.close()
    cfg = RoverEnvCfg(elevation=ElevationMapCfg())
    with pytest.raises(ValueError, match="camera"):
        cfg.validate()


def test_checkpoint_round_trip():
    """state_dict() -> a fresh env -> load_state_dict() -> one step: bit-identical extras and map."""
    a = _env()
    a.reset()
    for _ in range(3):
        _zero(a)
    sd = a.state_dict()
    assert {"elevation_map", "elevation_origin"} <= set(sd)
    b = _env()
    b.reset()
    b.load_state_dict(sd)
    _zero(a), _zero(b)
    for x, y in zip(_extras(a), _extras(b)):
        assert np.array_equal(_i32(x), _i32(y))
    assert torch.equal(a.sensors.elevation.map.view(torch.int32), b.sensors.elevation.map.view(torch.int32))
    assert torch.equal(a.sensors.elevation.origin, b.sensors.elevation.origin) and torch.isfinite(a.sensors.elevation.map).sum() > 1000
    a.close(), b.close()
