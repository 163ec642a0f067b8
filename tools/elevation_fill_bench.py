#!/usr/bin/env python3
"""What the elevation map's min-fill costs per env step, beside the two launches the map already has and a plain torch version.

    python tools/elevation_fill_bench.py --out profiles/elevation_fill_bench.json

Workload: 4096 envs on the config-2 terrain (procedural 2048^2 at 0.05 m, sigma_z 0.15 m, seed 1234, 400 rocks), G = 64 maps of
0.1 m cells, after ``--preroll`` untimed steps and ``--frames`` further steps that each feed the maps a frame (so the maps hold what
a running env's hold: the newest frame and what scrolled with the rover).  Two maps are filled on the same poses: one fed by the
160 x 90 camera through its sensor model, one by the dense lidar (64 channels, -85 .. -20 degrees, 1.5 degrees of azimuth).

Per map the items alternate in one process: ``rover_elevation_step`` with a frame, ``rover_elevation_scan``, ``rover_elevation_fill``
at 1, 8, 16, 32 and 64 iterations writing what the env's rig asks for (scan, column dist, count), the same at 32 iterations with
the two window outputs as well, and ``torch_fill`` below at 8, 16, 32 and 64 iterations.  A round is ``--calls`` back-to-back calls
under a host clock, ending in one device synchronise; the figure is the median over ``--reps`` rounds with min .. max.

``torch_fill`` is the same fill as unfused torch-ROCm ops: the window gathered out of the slot-addressed maps, one set of ops per
sweep (the masked 3 x 3 neighbourhood minimum as ``max_pool2d`` of the negated image, -inf where unknown), the scan columns
gathered out of the result.  It has no early exit (that would be a host synchronisation per sweep) and its minimum is a float
minimum, so -0 and +0 tie where the kernel orders them; the tool counts the cells whose bits differ.

Not attributed: the tool takes host-clock times of whole launches; how a fill launch divides into the window load, the sweeps and
the scan is read off the iteration sweep only (1 iteration is the load, one sweep and the scan; the slope over iterations is the
sweeps), not from counters or a kernel trace.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERATIONS = (8, 16, 32, 64)


def make_terrain(n):
    from isaac_rover_orbit_amd import terrain as T
    ter = T.make_procedural_terrain((2048, 2048), seed=1234, sigma_z=0.15, n_rocks=400)
    ter.make_spawns(2 * n, seed=41)
    return ter


def sensor_cfg():
    from isaac_rover_orbit_amd.cfg import DepthSensorCfg
    return DepthSensorCfg(range_min=0.3, range_max=8.0, sigma=(0.001, 0.0005, 0.002), p_drop=0.01, p_edge=0.4, disparity_step=0.125)


def summary(xs):
    return {"median_us": 1e6 * statistics.median(xs), "min_us": 1e6 * min(xs), "max_us": 1e6 * max(xs), "rounds": len(xs)}


def torch_fill(em, pos, quat, iterations):
    """``ElevationMap.fill`` in plain torch ops on ``em.map`` / ``em.origin``: returns (scan, column dist, count, filled window,
    cell dist), the last two in WINDOW order (n, G, G)."""
    import torch
    import torch.nn.functional as F
    c, n, G = em.cfg, em.num_envs, em.grid
    inf = float("inf")
    lo = em.origin.to(torch.int64) - G // 2
    w = torch.arange(G, device=lo.device)
    sy, sx = (lo[:, 1, None] + w) & (G - 1), (lo[:, 0, None] + w) & (G - 1)
    h = em.map.reshape(n, -1).gather(1, (sy[:, :, None] * G + sx[:, None, :]).reshape(n, -1)).reshape(n, G, G)
    dist = torch.where(torch.isnan(h), 255, 0).to(torch.uint8)
    for k in range(1, iterations + 1):
        unknown = torch.isnan(h)
        low = -F.max_pool2d(torch.where(unknown, -inf, -h)[:, None], 3, 1, 1)[:, 0]      # the padding counts as -inf
        take = unknown & (low < inf)
        h = torch.where(take, low, h)
        dist = torch.where(take, k, dist)
    w_, x, y, z = quat.unbind(1)
    a, b = 1 - 2 * (y * y + z * z), 2 * (w_ * z + x * y)
    inv = torch.rsqrt(a * a + b * b)
    cy, sn = (a * inv)[:, None, None], (b * inv)[:, None, None]
    ox, oy = em.ray_x[None, None, :], em.ray_y[None, :, None]
    px = pos[:, 0, None, None] + (cy * ox - sn * oy)
    py = pos[:, 1, None, None] + (sn * ox + cy * oy)
    rx = torch.floor(px * c.inv_cell).to(torch.int64) - lo[:, 0, None, None]
    ry = torch.floor(py * c.inv_cell).to(torch.int64) - lo[:, 1, None, None]
    inside = ((rx >= 0) & (rx < G) & (ry >= 0) & (ry < G)).reshape(n, -1)
    at = (ry.clamp(0, G - 1) * G + rx.clamp(0, G - 1)).reshape(n, -1)
    col_h, col_d = h.reshape(n, -1).gather(1, at), dist.reshape(n, -1).gather(1, at)
    col_d = torch.where(inside, col_d, 255)
    known = col_d < 255
    scan = torch.where(known, (pos[:, 2, None] - col_h) - c.height_offset, c.unknown_value)
    return scan, col_d, known.sum(1, dtype=torch.int32), h, dist


def window_order(em, t):
    """A slot-ordered (n, G, G) tensor in window order."""
    import torch
    n, G = em.num_envs, em.grid
    lo = em.origin.to(torch.int64) - G // 2
    w = torch.arange(G, device=lo.device)
    sy, sx = (lo[:, 1, None] + w) & (G - 1), (lo[:, 0, None] + w) & (G - 1)
    return t.reshape(n, -1).gather(1, (sy[:, :, None] * G + sx[:, None, :]).reshape(n, -1)).reshape(n, G, G)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--preroll", type=int, default=1500)
    ap.add_argument("--frames", type=int, default=8, help="steps after the pre-roll that feed the maps a frame each")
    ap.add_argument("--reps", type=int, default=9, help="rounds per item; the items alternate")
    ap.add_argument("--calls", type=int, default=20, help="calls per round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("elevation_fill_bench.py measures on a ROCm GPU; none is available")
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd.cfg import CameraCfg, ElevationMapCfg, LidarCfg, RoverEnvCfg
    from isaac_rover_orbit_amd.elevation import ElevationMap
    from isaac_rover_orbit_amd.envs import RoverEnv
    from isaac_rover_orbit_amd.lidar import Lidar, elevation_geometry, pattern_rays
    n, G = args.envs, args.grid
    cam = CameraCfg(sensor=sensor_cfg())
    cfg = RoverEnvCfg()
    cfg.scene.num_envs, cfg.terrain.kind = n, "custom"
    cfg.camera, cfg.elevation = cam, ElevationMapCfg(grid=G, range_min=0.3, range_max=8.0)
    env = RoverEnv(cfg, terrain=make_terrain(n))
    g = torch.Generator(device="cuda").manual_seed(0)
    actions = torch.rand(256, n, 2, device="cuda", generator=g) * 2 - 1
    env.reset()
    cam.every_n_steps, env.sensors.camera_every = 1 << 30, 1 << 30      # the pre-roll renders nothing
    em_cam, sensor = env.sensors.elevation, env.sensors.depth_sensor
    env.sensors.elevation = env.sensors.depth_sensor = None                    # the launches are made by hand below
    for k in range(args.preroll):
        env.step(actions[(k * 7) % 256])
    lidar_cfg = LidarCfg(channels=64, vertical_fov_range=(-85.0, -20.0), horizontal_res=1.5)
    lidar = Lidar(lidar_cfg, env, workspace=env.sensors.workspace)
    em_lid = ElevationMap(ElevationMapCfg(grid=G), elevation_geometry(lidar_cfg), cfg.height_scanner, n, "cuda", rays=pattern_rays(lidar_cfg))
    raw = torch.empty(n, cam.height, cam.width, device="cuda")
    img = torch.empty_like(raw)
    ranges = torch.empty(n, lidar.rays, device="cuda")
    pos, quat = env.state[_lib.POS:_lib.POS + 3].t(), env.state[_lib.QUAT:_lib.QUAT + 4].t()
    cols = em_cam.columns
    outs = (torch.empty(n, cols, device="cuda"), torch.empty(n, cols, dtype=torch.uint8, device="cuda"),
            torch.empty(n, dtype=torch.int32, device="cuda"))
    fouts = (torch.empty(n, cols, device="cuda"), torch.empty(n, cols, dtype=torch.uint8, device="cuda"),
             torch.empty(n, dtype=torch.int32, device="cuda"))
    filled, cell_dist = torch.empty(n, G, G, device="cuda"), torch.empty(n, G, G, dtype=torch.uint8, device="cuda")
    em_cam.clear()
    for k in range(args.frames):                                               # the maps gather frames along the way
        if k:
            env.step(actions[(k * 11) % 256])
        env.sensors.render_into(raw)
        sensor.apply(raw, 0, out=img)
        lidar.cast(ranges)
        em_cam.update(img, pos, quat, scan_out=outs[0], known_out=outs[1], count_out=outs[2])
        em_lid.update(ranges, pos, quat, scan_out=outs[0], known_out=outs[1], count_out=outs[2])
    torch.cuda.synchronize()
    pos_c, quat_c = pos.contiguous(), quat.contiguous()

    res = {"envs": n, "preroll": args.preroll, "frames": args.frames, "calls_per_round": args.calls, "grid": G, "cell": 0.1,
           "map_MB": n * G * G * 4 / 1e6, "sources": {}}
    for source, em, frame in (("camera", em_cam, img), ("lidar", em_lid, ranges)):
        em.scan(pos, quat, scan_out=outs[0], known_out=outs[1], count_out=outs[2])
        torch.cuda.synchronize()
        state = {"known_cell_share": float((~torch.isnan(em.map)).float().mean()), "measured_columns_mean": float(outs[2].float().mean()),
                 "fill": {}}
        for it in (1,) + ITERATIONS:
            em.fill(pos, quat, *fouts, filled_out=filled, cell_dist_out=cell_dist, iterations=it)
            t_scan, t_cd, t_count, t_h, t_dist = torch_fill(em, pos_c, quat_c, it)
            torch.cuda.synchronize()
            reached = cell_dist[cell_dist < 255]
            k_h = window_order(em, filled)
            both = (fouts[1] < 255) & (t_cd < 255)
            state["fill"][str(it)] = {
                "filled_columns_mean": float(fouts[2].float().mean()), "filled_columns_min": int(fouts[2].min()),
                "envs_with_all_columns": int((fouts[2] == cols).sum()), "largest_dist": int(reached.max()) if reached.numel() else 0,
                "filled_cell_share": float((cell_dist < 255).float().mean()),
                "torch_cell_dist_differs": int((window_order(em, cell_dist) != t_dist).sum()),
                "torch_cell_bits_differ": int(((k_h.view(torch.int32) != t_h.view(torch.int32)) & ~(torch.isnan(k_h) & torch.isnan(t_h))).sum()),
                "torch_column_dist_differs": int((fouts[1] != t_cd).sum()),
                "torch_max_abs_scan_diff_m": float((fouts[0] - t_scan)[both].abs().max()) if bool(both.any()) else 0.0}
        items = [("elevation_step", lambda: em.update(frame, pos, quat, scan_out=outs[0], known_out=outs[1], count_out=outs[2])),
                 ("elevation_scan", lambda: em.scan(pos, quat, scan_out=outs[0], known_out=outs[1], count_out=outs[2]))]
        items += [(f"fill_{it}", lambda it=it: em.fill(pos, quat, *fouts, iterations=it)) for it in (1,) + ITERATIONS]
        items += [("fill_32_with_window", lambda: em.fill(pos, quat, *fouts, filled_out=filled, cell_dist_out=cell_dist, iterations=32))]
        items += [(f"torch_fill_{it}", lambda it=it: torch_fill(em, pos_c, quat_c, it)) for it in ITERATIONS]
        for _, fn in items:
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        dt = {name: [] for name, _ in items}
        for _ in range(args.reps):
            for name, fn in items:
                calls = max(args.calls // 4, 1) if name.startswith("torch") else args.calls
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _k in range(calls):
                    fn()
                torch.cuda.synchronize()
                dt[name].append((time.perf_counter() - t0) / calls)
        state["time"] = {k: summary(v) for k, v in dt.items()}
        med = lambda k: state["time"][k]["median_us"]      # noqa: E731
        state["fill_32_over_step"] = med("fill_32") / med("elevation_step")
        state["fill_32_over_scan"] = med("fill_32") / med("elevation_scan")
        state["torch_over_fill"] = {str(it): med(f"torch_fill_{it}") / med(f"fill_{it}") for it in ITERATIONS}
        state["us_per_sweep_8_to_16"] = (med("fill_16") - med("fill_8")) / 8
        # what a fill launch must move: the maps read once, the scan rows, column dists and counts written
        state["traffic_floor_MB"] = n * (G * G * 4 + cols * 5 + 4) / 1e6
        state["floor_GB_per_s_at_fill_1"] = state["traffic_floor_MB"] / 1e3 / (med("fill_1") / 1e6)
        res["sources"][source] = state
    env.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
