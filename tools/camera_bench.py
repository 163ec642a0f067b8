"""Depth camera cost at the reference's scale: 4096 envs, 160 x 90 pixels, config-2 terrain (2048^2 fBm, 400 rocks).

    python tools/camera_bench.py [--envs 4096] [--warm 20] [--renders 200] [--steps 200] [--rounds 5] [--trace-only]

Prints one JSON line:
  render_ms        device-event time per rover_camera_render (median and spread over --rounds windows of --renders renders,
                   after --warm warm renders), on the states a 300-step pre-roll of random actions leaves
  grays_per_s      rays (= pixels) per second at the median
  out_bytes        bytes one render writes, and the write floor = out_bytes / 6.3 TB/s (measured HBM copy rate)
  step_ms_off/on   RoverEnv.step time without the camera and with a render after every step, the two envs alternated in windows
                   of --steps steps in one process (device events around each window)
--trace-only: warm up, then --renders renders and nothing else (for a rocprofv3 --kernel-trace --stats run of its own).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--renders", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--preroll", type=int, default=300)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("camera_bench needs the GPU")
    from isaac_rover_orbit_amd import terrain as T
    from isaac_rover_orbit_amd.cfg import CameraCfg, RoverEnvCfg
    from isaac_rover_orbit_amd.envs import RoverEnv

    n = a.envs
    ter = T.make_procedural_terrain((2048, 2048), seed=1234, sigma_z=0.15, n_rocks=400)
    ter.make_spawns(2 * n)

    def make(camera):
        cfg = RoverEnvCfg()
        cfg.scene.num_envs = n
        cfg.sim.device = "cuda:0"
        cfg.terrain.kind = "custom"
        cfg.camera = camera
        return RoverEnv(cfg, terrain=ter)

    on = make(CameraCfg())
    g = torch.Generator(device="cuda:0").manual_seed(0)
    on.reset()
    for _ in range(a.preroll):
        on.step(torch.rand(n, 2, device="cuda:0", generator=g) * 2 - 1)
    cam = on.cfg.camera
    buf = torch.empty(n, cam.height, cam.width, dtype=torch.float32, device="cuda:0")
    for _ in range(a.warm):
        on.sensors.render_into(buf)
    torch.cuda.synchronize()
    if a.trace_only:
        for _ in range(a.renders):
            on.sensors.render_into(buf)
        torch.cuda.synchronize()
        print(json.dumps({"trace_renders": a.renders, "envs": n}))
        return
    ms = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.renders):
            on.sensors.render_into(buf)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / a.renders)
    hit = float(torch.isfinite(buf).float().mean())
    med = statistics.median(ms)
    rays = n * cam.width * cam.height
    out_bytes = rays * 4

    off = make(None)
    off.reset()
    for _ in range(a.preroll):
        off.step(torch.rand(n, 2, device="cuda:0", generator=g) * 2 - 1)
    step = {"off": [], "on": []}
    for _ in range(a.rounds):
        for name, env in (("off", off), ("on", on)):
            acts = [torch.rand(n, 2, device="cuda:0", generator=g) * 2 - 1 for _ in range(a.steps)]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for x in acts:
                env.step(x)
            e1.record()
            e1.synchronize()
            step[name].append(e0.elapsed_time(e1) / a.steps)
    res = {
        "envs": n, "pixels": [cam.width, cam.height], "terrain": "2048^2 fBm sigma 0.15 m, 400 rocks",
        "render_ms": round(med, 4), "render_ms_rounds": [round(x, 4) for x in ms],
        "grays_per_s": round(rays / (med * 1e-3) / 1e9, 2), "hit_share": round(hit, 4),
        "out_bytes": out_bytes, "write_floor_us": round(out_bytes / 6.3e12 * 1e6, 1),
        "step_ms_off": round(statistics.median(step["off"]), 4), "step_ms_on": round(statistics.median(step["on"]), 4),
        "step_ms_off_rounds": [round(x, 4) for x in step["off"]], "step_ms_on_rounds": [round(x, 4) for x in step["on"]],
    }
    print(json.dumps(res))
    off.close()
    on.close()


if __name__ == "__main__":
    main()
