#!/usr/bin/env python3
"""Closed-loop evaluation of a trained actor (counterpart of the reference's examples/03_inference_pretrained/eval.py:
146-155): the skrl checkpoint's policy is packed once and evaluated by the fused MFMA kernel between env steps.

    python examples/03_eval_policy.py --checkpoint <.../policies/best_agent.pt> --num_envs 1024 --steps 750

``--scan_source elevation``: the actor reads its height scan out of a rolling elevation map built from the on-board depth camera
(``RoverEnvCfg.elevation``) in place of the oracle ray cast, so the same checkpoint runs on what the camera can see -- forward
only, through the sensor model of ``--depth_range`` / ``--depth_sigma`` / ``--depth_dropout``:

    python examples/03_eval_policy.py --checkpoint best_agent.pt --scan_source elevation --depth_range 0.3 8 --depth_dropout 0.01 0.4

``--map_source lidar`` builds that map from a scanning lidar on the mast instead (``RoverEnvCfg.lidar``, ``ElevationMapCfg.source``):
it sees all round, so the printed known share of the scan is close to 1 from the first frame on where the camera's stays low:

    python examples/03_eval_policy.py --checkpoint best_agent.pt --scan_source elevation --map_source lidar --lidar_channels 64 \
        --lidar_vfov -85 -20 --lidar_hres 1.5

``--map_fill min`` inpaints the map behind every update (``ElevationMapCfg.fill``): unknown cells take the minimum of their known
neighbours at most ``--map_fill_iterations`` cells far, the actor reads ``extras["elevation_scan_filled"]``, and the summary adds
the mean measured and filled column counts:

    python examples/03_eval_policy.py --checkpoint best_agent.pt --scan_source elevation --map_fill min --map_fill_iterations 20

``--map_cost`` derives slope, step height, roughness and a traversability cost from the map (from the filled window under
``--map_fill min``) over neighbourhoods of ``--map_cost_radius`` cells (``ElevationMapCfg.traverse``); the summary adds the mean
cost under the scan's columns and the mean number of lethal columns.  The actor's input does not change:

    python examples/03_eval_policy.py --checkpoint best_agent.pt --scan_source elevation --map_fill min --map_cost --map_cost_radius 2
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isaac_rover_orbit_amd import terrain as T  # noqa: E402
from isaac_rover_orbit_amd.cfg import RoverEnvCfg  # noqa: E402
from isaac_rover_orbit_amd.envs import RoverEnv  # noqa: E402
from isaac_rover_orbit_amd.policy import RoverNet  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--num_envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=750)
    ap.add_argument("--scan_source", choices=("raycast", "elevation"), default="raycast",
                    help="where the actor's height scan comes from: the oracle ray cast, or an elevation map built from the depth camera")
    ap.add_argument("--depth_range", type=float, nargs=2, default=None, metavar=("MIN", "MAX"),
                    help="the sensor's working range (m): depths outside it, misses included, carry no data")
    ap.add_argument("--depth_sigma", type=float, nargs=3, default=None, metavar=("S0", "S1", "S2"),
                    help="axial noise of standard deviation S0 + S1 z + S2 z^2 (m) at depth z")
    ap.add_argument("--depth_dropout", type=float, nargs=2, default=None, metavar=("P", "P_EDGE"),
                    help="probability that a pixel loses its data, off and on a depth edge")
    ap.add_argument("--map_alpha", type=float, default=1.0, help="weight of the newest frame on a cell the map already knows")
    ap.add_argument("--map_source", choices=("camera", "lidar"), default="camera",
                    help="the sensor that feeds the elevation map: the depth camera, or a scanning lidar on the mast")
    ap.add_argument("--map_fill", choices=("none", "min"), default="none",
                    help="inpaint the map behind every update: unknown cells take the minimum of their known neighbours, and the actor "
                         "reads the filled scan")
    ap.add_argument("--map_fill_iterations", type=int, default=32, metavar="N", help="how many cells far a height is carried at the most")
    ap.add_argument("--map_cost", action="store_true",
                    help="slope, step, roughness and cost layers behind every map update (needs --scan_source elevation); reported only")
    ap.add_argument("--map_cost_radius", type=int, default=2, metavar="R", help="the layers' neighbourhood is (2 R + 1)^2 cells, R in [1, 4]")
    ap.add_argument("--lidar_channels", type=int, default=32, help="rings of the lidar")
    ap.add_argument("--lidar_vfov", type=float, nargs=2, default=(-60.0, -10.0), metavar=("LO", "HI"),
                    help="elevation angles of the lowest and the highest ring (degrees)")
    ap.add_argument("--lidar_hres", type=float, default=2.0, help="degrees of azimuth between two rays of a ring")
    return ap


def make_cfg(args) -> RoverEnvCfg:
    """The env cfg of the flags: with ``--scan_source elevation`` the camera, its sensor model (None without a --depth_* flag) and
    the map -- or, with ``--map_source lidar``, the lidar of the ``--lidar_*`` flags and the map behind it; otherwise exactly the
    default."""
    if args.map_cost and args.scan_source != "elevation":
        raise ValueError("--map_cost needs --scan_source elevation")
    cfg = RoverEnvCfg()
    cfg.scene.num_envs = args.num_envs
    cfg.terrain.kind = "custom"
    if args.scan_source == "elevation" and args.map_source == "lidar":
        from isaac_rover_orbit_amd.cfg import ElevationMapCfg, LidarCfg
        cfg.lidar = LidarCfg(channels=args.lidar_channels, vertical_fov_range=tuple(args.lidar_vfov), horizontal_res=args.lidar_hres)
        cfg.elevation = ElevationMapCfg(alpha=args.map_alpha, source="lidar")
    elif args.scan_source == "elevation":
        from isaac_rover_orbit_amd.cfg import CameraCfg, DepthSensorCfg, ElevationMapCfg
        cfg.camera = CameraCfg()
        if any(v is not None for v in (args.depth_range, args.depth_sigma, args.depth_dropout)):
            s = cfg.camera.sensor = DepthSensorCfg()
            if args.depth_range is not None:
                s.range_min, s.range_max = args.depth_range
            if args.depth_sigma is not None:
                s.sigma = tuple(args.depth_sigma)
            if args.depth_dropout is not None:
                s.p_drop, s.p_edge = args.depth_dropout
        cfg.elevation = ElevationMapCfg(alpha=args.map_alpha)
    if cfg.elevation is not None:
        cfg.elevation.fill, cfg.elevation.fill_iterations = args.map_fill, args.map_fill_iterations
        if args.map_cost:
            from isaac_rover_orbit_amd.cfg import TraverseCfg
            cfg.elevation.traverse = TraverseCfg(radius=args.map_cost_radius)
    return cfg


def eval_on_map(env, actor, steps: int):
    """The loop of ``main`` with the actor on ``policy_rows(obs, extras["elevation_scan"])`` -- under ``--map_fill min`` on
    ``extras["elevation_scan_filled"]``; also the mean known share and the mean measured and filled column counts (the last
    ``None`` without a fill), and under ``--map_cost`` (mean cost of the columns that have one, mean lethal columns per scan), else
    ``None``."""
    from isaac_rover_orbit_amd.elevation import policy_rows
    obs, info = env.reset()
    counts, episodes, known, filled, cost, lethal = torch.zeros(4), 0.0, 0.0, 0.0, 0.0, 0.0
    rows = torch.empty_like(obs["policy"])
    key = "elevation_scan_filled" if "elevation_scan_filled" in info else "elevation_scan"
    for _ in range(steps):
        torch.nan_to_num_(obs["policy"], neginf=0.0)
        policy_rows(obs["policy"], info[key], out=rows)
        obs, rew, terminated, truncated, info = env.step(actor.act(rows))
        log = env.episode_log_vector.cpu()
        known += float(info["elevation_count"].float().mean())
        if "elevation_filled_count" in info:
            filled += float(info["elevation_filled_count"].float().mean())
        if "elevation_cost" in info:
            judged = info["elevation_cost_class"] > 0
            cost += float(info["elevation_cost"][judged].mean()) if bool(judged.any()) else 0.0
            lethal += float(info["elevation_lethal_count"].float().mean())
        if log[13] > 0:
            episodes += float(log[13])
            counts += log[7:11]
    steps = max(steps, 1)
    return (episodes, counts, known / steps / (rows.shape[1] - 4), (known / steps, filled / steps if "elevation_filled_count" in info else None),
            (cost / steps, lethal / steps) if "elevation_cost" in info else None)


def main():
    args = build_parser().parse_args()
    terrain = T.make_procedural_terrain((2048, 2048), seed=1234)
    terrain.make_spawns(2 * args.num_envs)
    env = RoverEnv(make_cfg(args), terrain=terrain)
    actor = RoverNet.from_checkpoint(args.checkpoint, role="policy")
    if args.scan_source == "elevation":
        episodes, counts, known, (measured, filled), cost = eval_on_map(env, actor, args.steps)
        print(f"episodes finished: {episodes:.0f}; terminations (time_out, success, far, collision): {counts.tolist()}; "
              f"mean known share of the scan: {known:.3f}")
        if filled is not None:
            print(f"mean measured columns per scan: {measured:.1f}; mean columns after the min-fill: {filled:.1f}")
        if cost is not None:
            print(f"mean cost of the columns with a verdict: {cost[0]:.3f}; mean lethal columns per scan: {cost[1]:.1f}")
        env.close()
        return
    obs, _ = env.reset()
    counts = torch.zeros(4)                              # time_out, is_success, far_from_target, collision
    episodes = 0.0
    for _ in range(args.steps):
        torch.nan_to_num_(obs["policy"], neginf=0.0)    # rays that leave the map report -inf (ORBIT RayCaster semantics)
        obs, rew, terminated, truncated, info = env.step(actor.act(obs))
        log = env.episode_log_vector.cpu()               # one small device -> host copy per step (this is an example)
        if log[13] > 0:
            episodes += float(log[13])
            counts += log[7:11]
    print(f"episodes finished: {episodes:.0f}; terminations (time_out, success, far, collision): {counts.tolist()}")
    env.close()


if __name__ == "__main__":
    main()
