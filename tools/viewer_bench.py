"""rgb_array viewer cost at the bench workload: 4096 envs on the config-2 terrain (2048^2 fBm, 400 rocks), one 1280 x 720 frame.

    python tools/viewer_bench.py [--envs 4096] [--warm 20] [--renders 100] [--rounds 5] [--preroll 300] [--trace-only]

Prints one JSON line; per origin mode ("world": the reference's eye (-6, -6, 3.5) looking at the origin; "env": 8 m behind and
4 m above env 0, looking at it):
  frame_ms      device-event time per render_rgb() (binning pass + render launch; median and spread over --rounds windows of
                --renders frames, after --warm warm frames) on the states a --preroll-step pre-roll of random actions leaves
  grays_per_s   rays (= pixels) per second at the median
  host_ms       render() wall time: the frame plus its 3.7 MB copy to the host (median of --renders)
--trace-only: warm up, then --renders frames of each mode and nothing else (for a rocprofv3 --kernel-trace --stats run of its own).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--renders", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--preroll", type=int, default=300)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("viewer_bench needs the GPU")
    from isaac_rover_orbit_amd import terrain as T
    from isaac_rover_orbit_amd.cfg import RoverEnvCfg, ViewerCfg
    from isaac_rover_orbit_amd.envs import RoverEnv

    n = a.envs
    ter = T.make_procedural_terrain((2048, 2048), seed=1234, sigma_z=0.15, n_rocks=400)
    ter.make_spawns(2 * n)
    cfg = RoverEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    cfg.terrain.kind = "custom"
    env = RoverEnv(cfg, terrain=ter, render_mode="rgb_array")
    g = torch.Generator(device="cuda:0").manual_seed(0)
    env.reset()
    for _ in range(a.preroll):
        env.step(torch.rand(n, 2, device="cuda:0", generator=g) * 2 - 1)
    modes = {"world": ViewerCfg(eye=(-6.0, -6.0, 3.5), lookat=(0.0, 0.0, 0.0)),
             "env": ViewerCfg(eye=(-8.0, 0.0, 4.0), lookat=(0.0, 0.0, 0.0), origin_type="env", env_index=0)}
    res = {"envs": n, "pixels": [1280, 720], "terrain": "2048^2 fBm sigma 0.15 m, 400 rocks"}
    for name, v in modes.items():
        env.cfg.viewer = v
        for _ in range(a.warm):
            env.render_rgb()
        torch.cuda.synchronize()
        if a.trace_only:
            for _ in range(a.renders):
                env.render_rgb()
            torch.cuda.synchronize()
            continue
        ms = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.renders):
                env.render_rgb()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.renders)
        host = []
        for _ in range(a.renders):
            t0 = time.perf_counter()
            env.render()
            host.append((time.perf_counter() - t0) * 1e3)
        _, _, ids = env.render_frame(object_id=True)
        med = statistics.median(ms)
        res[name] = {"frame_ms": round(med, 4), "frame_ms_rounds": [round(x, 4) for x in ms],
                     "grays_per_s": round(1280 * 720 / (med * 1e-3) / 1e9, 3), "host_ms": round(statistics.median(host), 3),
                     "rover_pixels": int((ids >= 3).sum())}
    if a.trace_only:
        res["trace_renders_per_mode"] = a.renders
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
