#!/usr/bin/env python3
"""What the rolling elevation map costs per env step, beside the camera launches in front of it and a plain torch version.

    python tools/elevation_bench.py --out profiles/elevation_bench.json

Workload: 4096 envs on the config-2 terrain (procedural 2048^2 at 0.05 m, sigma_z 0.15 m, seed 1234, 400 rocks) with the 160 x 90
camera and a G = 64 map of 0.1 m cells, after ``--preroll`` untimed steps (episodes of mixed age, the device at its sustained
clocks).  Four items alternate in one process on the same poses and images: the camera render (``rover_camera_render``), the depth
sensor model (``rover_depth_sensor_apply``, every stage on), the map's ONE launch (``rover_elevation_step``: scroll, unproject,
reduce, fuse, scan) and the same update as unfused torch-ROCm ops (``torch_step`` below: index arithmetic, ``scatter_reduce``
amax over 59 M points, gather).  A round is ``--calls`` back-to-back calls under a host clock, ending in one device synchronise; the
figure is the median over ``--reps`` rounds with min .. max.  The torch version runs on a copy of the map.

Traffic floor of the launch (bytes that must move): the images once (4096 x 14400 x 4 B), the maps read and written (4096 x 64 x
64 x 4 B x 2), the scan rows, known bytes and counts written.
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


def sensor_cfg():
    from isaac_rover_orbit_amd.cfg import DepthSensorCfg
    return DepthSensorCfg(range_min=0.3, range_max=8.0, sigma=(0.001, 0.0005, 0.002), p_drop=0.01, p_edge=0.4, disparity_step=0.125)


def summary(xs, per=1):
    return {"median_us": 1e6 * statistics.median(xs) / per, "min_us": 1e6 * min(xs) / per, "max_us": 1e6 * max(xs) / per, "rounds": len(xs)}


def torch_step(em, depth, pos, quat, mp, origin, reset=None):
    """``ElevationMap.update`` in plain torch ops (no reset of single envs unless ``reset`` (n,) bool is given): returns (scan,
    known, count) and updates ``mp`` (n, G, G) and ``origin`` (n, 2) in place.  Same semantics; the arithmetic is torch's own, so
    the heights agree to rounding, not to the bit."""
    import torch
    c, n, G = em.cfg, em.num_envs, em.grid
    nan, inf = float("nan"), float("inf")
    d = depth.reshape(n, -1)
    valid = torch.isfinite(d) & (d >= c.range_min) & (d <= c.range_max)
    mount = torch.tensor(list(c.mount_pos), device=d.device)
    b = mount + d[..., None] * em.rays                                          # (n, hw, 3)
    w, x, y, z = quat.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)
    pw = pos[:, None, :] + torch.bmm(b, R.transpose(1, 2))
    g = torch.floor(pw[..., :2] * c.inv_cell).to(torch.int64)
    centre = torch.floor(pos[:, :2] * c.inv_cell).to(torch.int64)
    lo = centre - G // 2
    rel = g - lo[:, None, :]
    inside = valid & torch.isfinite(pw).all(-1) & (rel >= 0).all(-1) & (rel < G).all(-1)
    slot = torch.where(inside, (g[..., 1] & (G - 1)) * G + (g[..., 0] & (G - 1)), G * G)       # G * G: the bin of the dropped
    frame = torch.full((n, G * G + 1), -inf, device=d.device)
    frame.scatter_reduce_(1, slot, pw[..., 2], "amax", include_self=True)
    frame = frame[:, :G * G].reshape(n, G, G)
    s = torch.arange(G, device=d.device)
    olo = origin.to(torch.int64) - G // 2
    same = [(lo[:, k, None] + ((s - lo[:, k, None]) & (G - 1))) == (olo[:, k, None] + ((s - olo[:, k, None]) & (G - 1))) for k in (0, 1)]
    keep = same[1][:, :, None] & same[0][:, None, :]
    if reset is not None:
        keep = keep & ~reset[:, None, None]
    old = torch.where(keep, mp, nan)
    fused = torch.where(torch.isnan(old), frame, old + c.alpha * (frame - old)) if c.alpha != 1.0 else frame
    mp.copy_(torch.where(frame > -inf, fused, old))
    origin.copy_(centre.to(torch.int32))
    a, bb = 1 - 2 * (y * y + z * z), 2 * (w * z + x * y)
    inv = torch.rsqrt(a * a + bb * bb)
    cy, sy = (a * inv)[:, None, None], (bb * inv)[:, None, None]
    ox, oy = em.ray_x[None, None, :], em.ray_y[None, :, None]
    sx_ = pos[:, 0, None, None] + (cy * ox - sy * oy)
    sy_ = pos[:, 1, None, None] + (sy * ox + cy * oy)
    gx, gy = torch.floor(sx_ * c.inv_cell).to(torch.int64), torch.floor(sy_ * c.inv_cell).to(torch.int64)
    rx, ry = gx - lo[:, 0, None, None], gy - lo[:, 1, None, None]
    h = mp.reshape(n, -1).gather(1, ((gy & (G - 1)) * G + (gx & (G - 1))).reshape(n, -1))
    known = ((rx >= 0) & (rx < G) & (ry >= 0) & (ry < G)).reshape(n, -1) & ~torch.isnan(h)
    scan = torch.where(known, (pos[:, 2, None] - h) - c.height_offset, c.unknown_value)
    return scan, known.to(torch.uint8), known.sum(1, dtype=torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--preroll", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=9, help="rounds per item; the items alternate")
    ap.add_argument("--calls", type=int, default=20, help="calls per round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("elevation_bench.py measures on a ROCm GPU; none is available")
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd.cfg import CameraCfg, ElevationMapCfg, RoverEnvCfg
    from isaac_rover_orbit_amd.envs import RoverEnv
    n = args.envs
    cam = CameraCfg(sensor=sensor_cfg())
    cfg = RoverEnvCfg()
    cfg.scene.num_envs, cfg.terrain.kind = n, "custom"
    cfg.camera, cfg.elevation = cam, ElevationMapCfg(grid=args.grid, range_min=0.3, range_max=8.0)
    env = RoverEnv(cfg, terrain=make_terrain(n))
    g = torch.Generator(device="cuda").manual_seed(0)
    actions = torch.rand(256, n, 2, device="cuda", generator=g) * 2 - 1
    env.reset()
    cam.every_n_steps, env.sensors.camera_every = 1 << 30, 1 << 30      # the pre-roll renders nothing
    em, sensor = env.sensors.elevation, env.sensors.depth_sensor
    env.sensors.elevation = env.sensors.depth_sensor = None                    # the launches are made by hand below
    for k in range(args.preroll):
        env.step(actions[(k * 7) % 256])
    raw = torch.empty(n, cam.height, cam.width, device="cuda")
    img = torch.empty_like(raw)
    pos, quat = env.state[_lib.POS:_lib.POS + 3].t(), env.state[_lib.QUAT:_lib.QUAT + 4].t()
    pos_c, quat_c = pos.contiguous(), quat.contiguous()
    outs = (torch.empty(n, em.columns, device="cuda"), torch.empty(n, em.columns, dtype=torch.uint8, device="cuda"),
            torch.empty(n, dtype=torch.int32, device="cuda"))
    env.sensors.render_into(raw)
    sensor.apply(raw, 0, out=img)
    em.update(img, pos, quat, scan_out=outs[0], known_out=outs[1], count_out=outs[2])       # the maps hold one frame
    t_map, t_origin = em.map.clone(), em.origin.clone()
    t_scan, t_known, t_count = torch_step(em, img, pos_c, quat_c, t_map, t_origin)
    torch.cuda.synchronize()
    both = outs[1].bool() & t_known.bool()
    agree = {"known_columns_differ": int((outs[1] != t_known).sum()), "known_share": float(outs[1].float().mean()),
             "max_abs_scan_diff_m": float((outs[0] - t_scan)[both].abs().max()),
             # torch rounds the unprojection its own way (bmm, rsqrt): a point on a cell border may land in the neighbour cell
             "share_of_known_columns_off_by_more_than_1e-4_m": float(((outs[0] - t_scan)[both].abs() > 1e-4).float().mean())}

    items = (("render", lambda: env.sensors.render_into(raw)),
             ("sensor", lambda: sensor.apply(raw, 0, out=img)),
             ("elevation_step", lambda: em.update(img, pos, quat, scan_out=outs[0], known_out=outs[1], count_out=outs[2])),
             ("elevation_step_no_frame", lambda: em.update(None, pos, quat, scan_out=outs[0], known_out=outs[1], count_out=outs[2])),
             ("torch_step", lambda: torch_step(em, img, pos_c, quat_c, t_map, t_origin)))
    for _, fn in items:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    dt = {name: [] for name, _ in items}
    for _ in range(args.reps):
        for name, fn in items:
            calls = max(args.calls // 4, 1) if name == "torch_step" else args.calls
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _k in range(calls):
                fn()
            torch.cuda.synchronize()
            dt[name].append((time.perf_counter() - t0) / calls)
    hw, G = cam.height * cam.width, em.grid
    res = {"envs": n, "preroll": args.preroll, "calls_per_round": args.calls, "image": [cam.height, cam.width], "grid": G, "cell": 0.1,
           "range": [0.3, 8.0], "agreement_with_torch": agree}
    res.update({k: summary(v) for k, v in dt.items()})
    res["torch_over_fused"] = res["torch_step"]["median_us"] / res["elevation_step"]["median_us"]
    res["traffic_floor_MB"] = n * (hw * 4 + G * G * 4 * 2 + em.columns * 5 + 4) / 1e6
    res["floor_GB_per_s_at_median"] = res["traffic_floor_MB"] / 1e3 / (res["elevation_step"]["median_us"] / 1e6)
    env.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
