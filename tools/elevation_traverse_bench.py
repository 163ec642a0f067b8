#!/usr/bin/env python3
"""What the elevation map's slope / step / roughness / cost launch costs per env step, beside the three launches the map already
has and a plain torch version.

    python tools/elevation_traverse_bench.py --out profiles/elevation_traverse_bench.json

Workload and protocol are those of tools/elevation_fill_bench.py: 4096 envs on the config-2 terrain, G = 64 maps of 0.1 m cells
after ``--preroll`` untimed steps and ``--frames`` further steps that each feed the maps a frame; one map fed by the 160 x 90 camera
through its sensor model, one by the dense lidar.  Per map the items alternate in one process; a round is ``--calls`` back-to-back
calls under a host clock, ending in one device synchronise; the figure is the median over ``--reps`` rounds with min .. max.

Items: ``rover_elevation_step`` with a frame, ``rover_elevation_scan``, ``rover_elevation_fill`` at 32 iterations (with the window
output the rig asks for under traverse), and ``rover_elevation_traverse`` on the map at r = 1, 2 and 4
  * writing what the env's rig asks for (cost scan, column class, lethal count): the sparse form, a verdict only for the cells
    under the scan's columns;
  * with the cost window as well, and with all four window outputs: the dense form, a verdict for every cell;
and at r = 2 on the fill's window instead of the map; and ``torch_traverse`` below at r = 1, 2 and 4.

``torch_traverse`` is the same layers as unfused torch-ROCm ops: the window gathered out of the slot-addressed maps, the extrema as
``max_pool2d`` of the masked image, the neighbourhood of every cell as ``unfold`` for support and roughness, elementwise ops for
the rest, the scan columns gathered out of the result.  Its roughness sums in torch's reduction order and its extrema are float
extrema, so it need not agree in the bits; the tool counts the cells whose class differs and reports the largest cost difference.

Not attributed: the tool takes host-clock times of whole launches; how a traverse launch divides into the window load, the
verdicts, the window stores and the scan is read off the items' differences only, not from counters or a kernel trace.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

RADII = (1, 2, 4)


def torch_traverse(em, pos, quat, t, heights=None):
    """``ElevationMap.traverse`` in plain torch ops: returns (cost scan, column class, lethal count, slope, step, rough, cost, class),
    the last five in WINDOW order (n, G, G)."""
    import torch
    import torch.nn.functional as F
    from elevation_fill_bench import window_order
    c, n, G, r = em.cfg, em.num_envs, em.grid, int(t.radius)
    k, inf, nan = 2 * r + 1, float("inf"), float("nan")
    h = window_order(em, em.map if heights is None else heights)
    ok = torch.isfinite(h)
    hi = F.max_pool2d(torch.where(ok, h, -inf)[:, None], k, 1, r)[:, 0]                  # the padding counts as -inf
    lo = -F.max_pool2d(torch.where(ok, -h, -inf)[:, None], k, 1, r)[:, 0]
    step = hi - lo
    hp = F.pad(h[:, None], (1, 1, 1, 1), value=nan)[:, 0]

    def one_sided(lower, upper):
        l, u = torch.isfinite(lower), torch.isfinite(upper)
        return torch.where(l & u, (upper - lower) * (0.5 * c.inv_cell),
                           torch.where(u, (upper - h) * c.inv_cell, torch.where(l, (h - lower) * c.inv_cell, 0.0)))

    gx, gy = one_sided(hp[:, 1:-1, :-2], hp[:, 1:-1, 2:]), one_sided(hp[:, :-2, 1:-1], hp[:, 2:, 1:-1])
    slope = torch.sqrt(gx * gx + gy * gy)
    near = F.unfold(F.pad(h[:, None], (r, r, r, r), value=nan), k)                     # (n, k * k, G * G): di outer, dj inner
    near_ok = torch.isfinite(near)
    support = near_ok.sum(1).reshape(n, G, G)
    d = torch.arange(-r, r + 1, device=h.device, dtype=torch.float32) * c.cell
    dy, dx = d.repeat_interleave(k)[None, :, None], d.repeat(k)[None, :, None]
    res = (near - h.reshape(n, 1, -1)) - (gx.reshape(n, 1, -1) * dx + gy.reshape(n, 1, -1) * dy)
    near_ok[:, (k * k) // 2] = False                                                    # the centre
    acc = torch.where(near_ok, res * res, 0.0).sum(1).reshape(n, G, G)
    cnt = support - 1
    rough = torch.where(cnt > 0, torch.sqrt(acc / cnt.clamp(min=1)), 0.0)
    lethal = ~((slope < t.slope_crit) & (step < t.step_crit) & (rough < t.rough_crit))
    total = t.w_slope * (slope / t.slope_crit) + t.w_step * (step / t.step_crit) + t.w_rough * (rough / t.rough_crit)
    cost = torch.where(lethal, 1.0, total.clamp(max=1.0))
    verdict = ok & (support >= t.min_support)
    cls = torch.where(verdict, torch.where(lethal, 2, 1), 0).to(torch.uint8)
    slope, step, rough, cost = (torch.where(verdict, a, nan) for a in (slope, step, rough, cost))
    w_, x, y, z = quat.unbind(1)
    a, b = 1 - 2 * (y * y + z * z), 2 * (w_ * z + x * y)
    inv = torch.rsqrt(a * a + b * b)
    cy, sn = (a * inv)[:, None, None], (b * inv)[:, None, None]
    ox, oy = em.ray_x[None, None, :], em.ray_y[None, :, None]
    px = pos[:, 0, None, None] + (cy * ox - sn * oy)
    py = pos[:, 1, None, None] + (sn * ox + cy * oy)
    low = em.origin.to(torch.int64) - G // 2
    rx = torch.floor(px * c.inv_cell).to(torch.int64) - low[:, 0, None, None]
    ry = torch.floor(py * c.inv_cell).to(torch.int64) - low[:, 1, None, None]
    inside = ((rx >= 0) & (rx < G) & (ry >= 0) & (ry < G)).reshape(n, -1)
    at = (ry.clamp(0, G - 1) * G + rx.clamp(0, G - 1)).reshape(n, -1)
    col_cls = torch.where(inside, cls.reshape(n, -1).gather(1, at), 0).to(torch.uint8)
    scan = torch.where(col_cls > 0, cost.reshape(n, -1).gather(1, at), t.unknown_cost)
    return scan, col_cls, (col_cls == 2).sum(1, dtype=torch.int32), slope, step, rough, cost, cls


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
        raise SystemExit("elevation_traverse_bench.py measures on a ROCm GPU; none is available")
    from elevation_fill_bench import make_terrain, sensor_cfg, summary, window_order
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd.cfg import CameraCfg, ElevationMapCfg, LidarCfg, RoverEnvCfg, TraverseCfg
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
    mk = lambda: (torch.empty(n, cols, device="cuda"), torch.empty(n, cols, dtype=torch.uint8, device="cuda"),      # noqa: E731
                  torch.empty(n, dtype=torch.int32, device="cuda"))
    outs, fouts, touts = mk(), mk(), mk()
    filled = torch.empty(n, G, G, device="cuda")
    layers = [torch.empty(n, G, G, device="cuda") for _ in range(4)]
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
    tcfg = {r: TraverseCfg(radius=r) for r in RADII}
    names = ("scan_out", "class_out", "count_out")

    res = {"envs": n, "preroll": args.preroll, "frames": args.frames, "calls_per_round": args.calls, "grid": G, "cell": 0.1,
           "map_MB": n * G * G * 4 / 1e6, "traverse_cfg": {k: v for k, v in TraverseCfg().__dict__.items() if k != "radius"}, "sources": {}}
    for source, em, frame in (("camera", em_cam, img), ("lidar", em_lid, ranges)):
        em.scan(pos, quat, scan_out=outs[0], known_out=outs[1], count_out=outs[2])
        em.fill(pos, quat, *fouts, filled_out=filled, iterations=32)
        torch.cuda.synchronize()
        state = {"known_cell_share": float((~torch.isnan(em.map)).float().mean()), "measured_columns_mean": float(outs[2].float().mean()),
                 "filled_columns_mean": float(fouts[2].float().mean()), "layers": {}}
        for r in RADII:
            em.traverse(pos, quat, **dict(zip(names, touts)), slope_out=layers[0], step_out=layers[1], rough_out=layers[2],
                        cost_out=layers[3], cfg=tcfg[r])
            sparse = em.traverse(pos, quat, cfg=tcfg[r])
            t_scan, t_cls, t_count, _, _, _, t_cost, t_cell = torch_traverse(em, pos_c, quat_c, tcfg[r])
            torch.cuda.synchronize()
            k_cost = window_order(em, layers[3])
            judged = ~torch.isnan(k_cost)
            both = judged & ~torch.isnan(t_cost)
            state["layers"][str(r)] = {
                "cells_with_a_verdict_share": float(judged.float().mean()),
                "lethal_cell_share_of_those": float((k_cost[judged] == 1.0).float().mean()) if bool(judged.any()) else 0.0,
                "columns_with_a_cost_mean": float((touts[1] > 0).sum(1).float().mean()), "lethal_columns_mean": float(touts[2].float().mean()),
                "mean_cost_of_those_columns": float(touts[0][touts[1] > 0].mean()) if bool((touts[1] > 0).any()) else 0.0,
                "sparse_equals_dense_bits": bool(torch.equal(sparse[0].view(torch.int32), touts[0].view(torch.int32)) and
                                                 torch.equal(sparse[1], touts[1]) and torch.equal(sparse[2], touts[2])),
                "torch_cell_verdict_differs": int((judged != ~torch.isnan(t_cost)).sum()),
                "torch_cell_class_differs": int(((k_cost == 1.0) != (t_cost == 1.0))[both].sum()), "cells": int(judged.numel()),
                "torch_cell_cost_bits_differ": int((k_cost.view(torch.int32) != t_cost.view(torch.int32))[both].sum()),
                "torch_max_abs_cost_diff": float((k_cost - t_cost)[both].abs().max()) if bool(both.any()) else 0.0,
                "torch_column_class_differs": int((touts[1] != t_cls).sum()),
                "torch_lethal_count_differs_envs": int((touts[2] != t_count).sum())}
        items = [("elevation_step", lambda: em.update(frame, pos, quat, scan_out=outs[0], known_out=outs[1], count_out=outs[2])),
                 ("elevation_scan", lambda: em.scan(pos, quat, scan_out=outs[0], known_out=outs[1], count_out=outs[2])),
                 ("fill_32", lambda: em.fill(pos, quat, *fouts, iterations=32)),
                 ("fill_32_with_window", lambda: em.fill(pos, quat, *fouts, filled_out=filled, iterations=32))]
        items += [(f"traverse_r{r}", lambda r=r: em.traverse(pos, quat, **dict(zip(names, touts)), cfg=tcfg[r])) for r in RADII]
        items += [(f"traverse_r{r}_cost_window", lambda r=r: em.traverse(pos, quat, **dict(zip(names, touts)), cost_out=layers[3], cfg=tcfg[r]))
                  for r in RADII]
        items += [(f"traverse_r{r}_four_windows", lambda r=r: em.traverse(
            pos, quat, **dict(zip(names, touts)), slope_out=layers[0], step_out=layers[1], rough_out=layers[2], cost_out=layers[3], cfg=tcfg[r]))
            for r in RADII]
        items += [("traverse_r2_on_filled", lambda: em.traverse(pos, quat, heights=filled, **dict(zip(names, touts)), cfg=tcfg[2])),
                  ("traverse_r2_on_filled_cost_window", lambda: em.traverse(pos, quat, heights=filled, **dict(zip(names, touts)),
                                                                            cost_out=layers[3], cfg=tcfg[2]))]
        items += [(f"torch_traverse_r{r}", lambda r=r: torch_traverse(em, pos_c, quat_c, tcfg[r])) for r in RADII]
        em.fill(pos, quat, *fouts, filled_out=filled, iterations=32)
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
        state["torch_over_traverse_four_windows"] = {str(r): med(f"torch_traverse_r{r}") / med(f"traverse_r{r}_four_windows") for r in RADII}
        state["traverse_r2_over_step"] = med("traverse_r2") / med("elevation_step")
        state["traverse_r2_over_scan"] = med("traverse_r2") / med("elevation_scan")
        state["traverse_r2_over_fill_32"] = med("traverse_r2") / med("fill_32")
        state["dense_over_sparse"] = {str(r): med(f"traverse_r{r}_cost_window") / med(f"traverse_r{r}") for r in RADII}
        # what a launch must move: the heights read once, the scan rows, column classes and counts written; each window output on top
        scan_MB, window_MB = n * (G * G * 4 + cols * 5 + 4) / 1e6, n * G * G * 4 / 1e6
        state["traffic_floor_MB"] = {"scan_only": scan_MB, "cost_window": scan_MB + window_MB, "four_windows": scan_MB + 4 * window_MB}
        state["floor_TB_per_s"] = {
            **{f"traverse_r{r}": scan_MB / med(f"traverse_r{r}") for r in RADII},
            **{f"traverse_r{r}_cost_window": (scan_MB + window_MB) / med(f"traverse_r{r}_cost_window") for r in RADII},
            **{f"traverse_r{r}_four_windows": (scan_MB + 4 * window_MB) / med(f"traverse_r{r}_four_windows") for r in RADII}}      # MB / us
        res["sources"][source] = state
    env.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
