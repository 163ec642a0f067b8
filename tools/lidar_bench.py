#!/usr/bin/env python3
"""What a lidar frame costs, beside the camera's render, and whether a ring per wave beats a shuffled table.

    python tools/lidar_bench.py --out profiles/lidar_bench.json

Workload: 4096 envs on the config-2 terrain (procedural 2048^2 at 0.05 m, sigma_z 0.15 m, seed 1234, 400 rocks) after ``--preroll``
untimed steps (episodes of mixed age, the device at its sustained clocks).  Items alternate in one process on the same poses:

  lidar_default      ``rover_lidar_cast`` of the default pattern (32 x 180 = 5760 rays, channel-major: a wave holds one ring)
  lidar_dense        ... of the dense pattern (64 channels over -85 .. -20 degrees, 1.5 degrees of azimuth: 15360 rays)
  lidar_dense_shuffled   the same 15360 directions in a seeded random order: every wave holds 64 rays of mixed elevation and azimuth.
                     Same rays, same ranges (checked below, as a permutation), so the difference is the wave-to-ray mapping alone
  camera_render      ``rover_camera_render`` of the 160 x 90 image (14400 rays per env, 8 x 8 pixel tiles per wave)
  elevation_step     ``rover_elevation_step`` on the dense lidar frame (G = 64, 0.1 m cells)

A round is ``--calls`` back-to-back calls under a host clock, ending in one device synchronise; the figure is the median over
``--reps`` rounds with min .. max, and rays per second at the median.  Nothing is fixed in advance: the JSON carries what was measured.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_terrain(n):
    from isaac_rover_orbit_amd import terrain as T
    ter = T.make_procedural_terrain((2048, 2048), seed=1234, sigma_z=0.15, n_rocks=400)
    ter.make_spawns(2 * n, seed=41)
    return ter


def summary(xs, rays):
    med = statistics.median(xs)
    return {"median_us": 1e6 * med, "min_us": 1e6 * min(xs), "max_us": 1e6 * max(xs), "rounds": len(xs), "rays_per_launch": rays,
            "G_rays_per_s_at_median": rays / med / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--preroll", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=9, help="rounds per item; the items alternate")
    ap.add_argument("--calls", type=int, default=20, help="calls per round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lidar_bench.py measures on a ROCm GPU; none is available")
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd.cfg import CameraCfg, ElevationMapCfg, LidarCfg, RoverEnvCfg
    from isaac_rover_orbit_amd.elevation import ElevationMap
    from isaac_rover_orbit_amd.envs import RoverEnv
    from isaac_rover_orbit_amd.lidar import Lidar, elevation_geometry, pattern_rays
    n = args.envs
    cam = CameraCfg()
    cfg = RoverEnvCfg()
    cfg.scene.num_envs, cfg.terrain.kind, cfg.camera = n, "custom", cam
    env = RoverEnv(cfg, terrain=make_terrain(n))
    g = torch.Generator(device="cuda").manual_seed(0)
    actions = torch.rand(256, n, 2, device="cuda", generator=g) * 2 - 1
    env.reset()
    cam.every_n_steps, env.sensors.camera_every = 1 << 30, 1 << 30      # the pre-roll renders nothing
    for k in range(args.preroll):
        env.step(actions[(k * 7) % 256])
    # the three tables; every Lidar adopts the camera's prepared workspace (one pyramid per handle)
    default_cfg = LidarCfg()
    dense_cfg = LidarCfg(channels=64, vertical_fov_range=(-85.0, -20.0), horizontal_res=1.5)
    default, dense, shuffled = (Lidar(c, env, workspace=env.sensors.workspace) for c in (default_cfg, dense_cfg, dense_cfg))
    perm = np.random.default_rng(0).permutation(dense.rays)
    shuffled.table = torch.from_numpy(np.ascontiguousarray(pattern_rays(dense_cfg)[perm])).cuda()
    r_default = torch.empty(n, default.rays, device="cuda")
    r_dense, r_shuffled = torch.empty(n, dense.rays, device="cuda"), torch.empty(n, dense.rays, device="cuda")
    image = torch.empty(n, cam.height, cam.width, device="cuda")
    em = ElevationMap(ElevationMapCfg(), elevation_geometry(dense_cfg), cfg.height_scanner, n, "cuda", rays=pattern_rays(dense_cfg))
    pos, quat = env.state[_lib.POS:_lib.POS + 3].t(), env.state[_lib.QUAT:_lib.QUAT + 4].t()
    outs = (torch.empty(n, em.columns, device="cuda"), torch.empty(n, em.columns, dtype=torch.uint8, device="cuda"),
            torch.empty(n, dtype=torch.int32, device="cuda"))
    dense.cast(r_dense)
    shuffled.cast(r_shuffled)
    default.cast(r_default)
    em.update(r_dense, pos, quat, scan_out=outs[0], known_out=outs[1], count_out=outs[2])
    torch.cuda.synchronize()
    same = r_dense[:, torch.from_numpy(perm).cuda()]
    agree = {"shuffled_is_a_permutation_of_ring_order_bit_for_bit": bool(torch.equal(same.view(torch.int32), r_shuffled.view(torch.int32))),
             "hit_share_default": float(torch.isfinite(r_default).float().mean()),
             "hit_share_dense": float(torch.isfinite(r_dense).float().mean()),
             "mean_range_dense_m": float(r_dense[torch.isfinite(r_dense)].mean()),
             "known_columns_after_one_dense_frame_mean": float(outs[2].float().mean())}

    items = (("lidar_default", lambda: default.cast(r_default), n * default.rays),
             ("lidar_dense", lambda: dense.cast(r_dense), n * dense.rays),
             ("lidar_dense_shuffled", lambda: shuffled.cast(r_shuffled), n * dense.rays),
             ("camera_render", lambda: env.sensors.render_into(image), n * cam.height * cam.width),
             ("elevation_step", lambda: em.update(r_dense, pos, quat, scan_out=outs[0], known_out=outs[1], count_out=outs[2]),
              n * dense.rays))
    for _, fn, _ in items:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    dt = {name: [] for name, _, _ in items}
    for _ in range(args.reps):
        for name, fn, _ in items:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _k in range(args.calls):
                fn()
            torch.cuda.synchronize()
            dt[name].append((time.perf_counter() - t0) / args.calls)
    res = {"envs": n, "preroll": args.preroll, "calls_per_round": args.calls, "default_pattern": [default.channels, default.azimuths],
           "dense_pattern": [dense.channels, dense.azimuths], "camera_image": [cam.height, cam.width], "checks": agree}
    res.update({name: summary(dt[name], rays) for name, _, rays in items})
    ring, mixed = res["lidar_dense"]["median_us"], res["lidar_dense_shuffled"]["median_us"]
    res["shuffled_over_ring"] = mixed / ring
    res["ring_order_beat_shuffled"] = bool(res["lidar_dense"]["max_us"] < res["lidar_dense_shuffled"]["min_us"])
    res["lidar_dense_over_camera_rays_per_s"] = (res["lidar_dense"]["G_rays_per_s_at_median"] /
                                                 res["camera_render"]["G_rays_per_s_at_median"])
    env.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
