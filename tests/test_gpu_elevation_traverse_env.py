"""RoverEnv with ``ElevationMapCfg.traverse`` on the MI355X: the traverse launch behind every map update (and behind the fill where
there is one), on flat ground, against an env without it."""
import math

import numpy as np
import pytest
import torch

from helpers import flat
from isaac_rover_orbit_amd.cfg import CameraCfg, ElevationMapCfg, RoverEnvCfg, TraverseCfg
from lidar_cases import dense_cfg

pytestmark = pytest.mark.gpu

N = 4
KEYS = ("elevation_scan", "elevation_known", "elevation_count")
FILL_KEYS = ("elevation_scan_filled", "elevation_fill_dist", "elevation_filled_count")
TRAVERSE_KEYS = ("elevation_cost", "elevation_cost_class", "elevation_lethal_count")


def _env(traverse, source, fill):
    from isaac_rover_orbit_amd.envs import RoverEnv
    cfg = RoverEnvCfg()
    cfg.scene.num_envs = N
    cfg.sim.device = "cuda:0"
    cfg.terrain.kind = "custom"
    if source == "camera":
        cfg.camera = CameraCfg()
    else:
        cfg.lidar = dense_cfg()
    cfg.elevation = ElevationMapCfg(source=source, fill=fill, fill_iterations=64, traverse=traverse)
    return RoverEnv(cfg, terrain=flat())


def _zero(env):
    return env.step(torch.zeros(N, 2, device=env.device))


def _bits(t):
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view(np.int32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("fill", ["none", "min"])
@pytest.mark.parametrize("source", ["camera", "lidar"])
def test_the_cost_scan_on_flat_ground(source, fill):
    """reset() and two zero-action steps, after each: the three keys with their shapes and dtypes; every column the map knows (with
    a fill: every column with fill_dist < 255) is class 1; no lethal column; the older keys carry the bits of a twin env without
    traverse on the same seed and actions.  The cost bound: on flat ground a known column is within eps = 1e-4 range_max + 1e-4 m
    of the oracle (the bound of the raw and of the filled scan's own tests), so heights differ by at most 2 eps: slope <= sqrt(2)
    eps / cell with the centred difference, step <= 2 eps, rough <= 2 eps (1 + r), and the cost is their weighted sum of ratios."""
    t = TraverseCfg()
    a, b = _env(t, source, fill), _env(None, source, fill)
    assert a.sensors.traverse is t and b.sensors.traverse is None and not hasattr(b.sensors, "_costs")
    (_, extras), (_, twin) = a.reset(), b.reset()
    eps = 1e-4 * a.cfg.elevation.range_max + 1e-4
    cell = a.cfg.elevation.cell
    bound = t.w_slope * (math.sqrt(2) * eps / cell) / t.slope_crit + t.w_step * 2 * eps / t.step_crit + \
        t.w_rough * 2 * eps * (1 + t.radius) / t.rough_crit
    older = KEYS + (FILL_KEYS if fill == "min" else ())
    for s in range(3):
        if s:
            _, _, _, _, extras = _zero(a)
            _, _, _, _, twin = _zero(b)
        torch.cuda.synchronize()
        assert extras["elevation_cost"].shape == (N, 961) and extras["elevation_cost"].dtype == torch.float32
        assert extras["elevation_cost_class"].shape == (N, 961) and extras["elevation_cost_class"].dtype == torch.uint8
        assert extras["elevation_lethal_count"].shape == (N,) and extras["elevation_lethal_count"].dtype == torch.int32
        assert not any(k in twin for k in TRAVERSE_KEYS)
        for key in older:
            assert np.array_equal(_bits(extras[key]), _bits(twin[key])), (s, key)
        assert torch.equal(a.sensors.elevation.map.view(torch.int32), b.sensors.elevation.map.view(torch.int32))
        cost, cls, lethal = (extras[k].cpu().numpy() for k in TRAVERSE_KEYS)
        has = (extras["elevation_fill_dist"].cpu().numpy() < 255) if fill == "min" else (extras["elevation_known"].cpu().numpy() == 1)
        assert has.any(axis=1).all() and np.array_equal(cls == 1, has) and not (cls == 2).any() and not lethal.any()
        assert (cost[~has] == t.unknown_cost).all()
        top = float(cost[has].max())
        print(f"{source}, fill {fill}, step {s}: {has.sum(1).tolist()} columns with a cost, largest {top:.3e} (bound {bound:.3e})")
        assert 0.0 <= top <= bound
    assert set(a.state_dict()) == set(b.state_dict())                      # traverse has no state
    a.close(), b.close()
