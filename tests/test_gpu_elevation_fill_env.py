"""RoverEnv with ``ElevationMapCfg.fill = "min"`` on the MI355X: the fill launch behind every map update, on flat ground, against
the oracle scan and against an env without the fill."""
import numpy as np
import pytest
import torch

from helpers import flat
from isaac_rover_orbit_amd.cfg import CameraCfg, ElevationMapCfg, RoverEnvCfg
from lidar_cases import dense_cfg

pytestmark = pytest.mark.gpu

N = 8
KEYS = ("elevation_scan", "elevation_known", "elevation_count")
FILL_KEYS = ("elevation_scan_filled", "elevation_fill_dist", "elevation_filled_count")


def _env(fill, source="camera"):
    from isaac_rover_orbit_amd.envs import RoverEnv
    cfg = RoverEnvCfg()
    cfg.scene.num_envs = N
    cfg.sim.device = "cuda:0"
    cfg.terrain.kind = "custom"
    if source == "camera":
        cfg.camera = CameraCfg()
    else:
        cfg.lidar = dense_cfg()
    # 64 sweeps >= G - 1 = 63: the whole window fills whenever one cell of it is known (a property of the rule)
    cfg.elevation = ElevationMapCfg(source=source, fill=fill, fill_iterations=64)
    return RoverEnv(cfg, terrain=flat())


def _zero(env):
    return env.step(torch.zeros(N, 2, device=env.device))


def _bits(t):
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view(np.int32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("source", ["camera", "lidar"])
def test_the_filled_scan_on_flat_ground(source):
    """reset() and three zero-action steps, after each: every column is filled wherever one is measured; dist is 0 exactly on the
    measured columns; the filled scan agrees with the observation's oracle columns within 1e-4 * range_max + 1e-4 m (the
    flat-ground bound of the raw scan: a filled value is a measured cell's); the three old keys carry the bits of an env without the
    fill on the same seed and actions."""
    a, b = _env("min", source), _env("none", source)
    assert a.sensors.fill_iterations == 64 and b.sensors.fill_iterations == 0
    (obs, extras), _ = a.reset(), b.reset()
    bound = 1e-4 * a.cfg.elevation.range_max + 1e-4
    for s in range(4):
        if s:
            obs, _, _, _, extras = _zero(a)
            _zero(b)
        torch.cuda.synchronize()
        assert extras["elevation_scan_filled"].shape == (N, 961) and extras["elevation_scan_filled"].dtype == torch.float32
        assert extras["elevation_fill_dist"].shape == (N, 961) and extras["elevation_fill_dist"].dtype == torch.uint8
        assert extras["elevation_filled_count"].shape == (N,) and extras["elevation_filled_count"].dtype == torch.int32
        for key in KEYS:
            assert np.array_equal(_bits(a.extras[key]), _bits(b.extras[key])), (s, key)
        assert torch.equal(a.sensors.elevation.map.view(torch.int32), b.sensors.elevation.map.view(torch.int32))
        filled, dist, count = (extras[k].cpu().numpy() for k in FILL_KEYS)
        known, raw_count = extras["elevation_known"].cpu().numpy(), extras["elevation_count"].cpu().numpy()
        assert (raw_count > 0).all() and (count[raw_count > 0] == 961).all()
        assert np.array_equal(dist == 0, known == 1) and (dist < 255).all()
        assert source == "lidar" or (dist > 0).any()                       # the camera leaves holes; the dense lidar may not
        oracle = obs["policy"][:, 4:].cpu().numpy()
        assert np.isfinite(oracle).all()
        err = np.abs(filled.astype(np.float64) - oracle.astype(np.float64)).max()
        print(f"{source} step {s}: measured {raw_count.tolist()}, largest dist {dist.max()}, largest |filled - oracle| {err:.3e} m "
              f"(bound {bound:.1e})")
        assert err <= bound
        measured = dist == 0
        assert np.array_equal(_bits(extras["elevation_scan_filled"])[measured], _bits(extras["elevation_scan"])[measured])
    assert set(a.state_dict()) == set(b.state_dict())                      # the fill has no state
    a.close(), b.close()


def test_a_forced_reset_refills_and_no_fill_publishes_nothing():
    a = _env("min")
    a.reset()
    _zero(a)
    before = a.extras["elevation_scan_filled"]
    tries = a._native_cfg.max_target_tries
    rng = np.random.default_rng(3)
    mask = np.zeros(N, np.uint8)
    mask[2] = 1
    a.reset_with_draws(mask, np.arange(N, dtype=np.int32), rng.random(N).astype(np.float32), rng.random((N, tries)).astype(np.float32),
                       rng.random(N).astype(np.float32))
    torch.cuda.synchronize()
    assert a.extras["elevation_scan_filled"].data_ptr() != before.data_ptr()        # a launch of its own into the next buffers
    count, raw = a.extras["elevation_filled_count"].cpu().numpy(), a.extras["elevation_count"].cpu().numpy()
    assert (raw > 0).all() and (count == 961).all() and raw[2] < 961
    a.close()
    b = _env("none")
    _, extras = b.reset()
    _, _, _, _, extras = _zero(b)
    assert not any(k in extras for k in FILL_KEYS) and all(k in extras for k in KEYS) and not hasattr(b.sensors, "_fills")
    b.close()
