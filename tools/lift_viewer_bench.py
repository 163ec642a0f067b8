"""rgb_array viewer cost of FrankaCubeLift-v0 at the bench workload: 4096 envs (64 x 64 lattice, spacing 2.5 m), one 1280 x 720 frame.

    python tools/lift_viewer_bench.py [--envs 4096] [--warm 20] [--renders 100] [--rounds 5] [--preroll 100] [--trace-only]

Prints one JSON line; per origin mode ("world": the reference's eye (-6, -6, 3.5) looking at the origin; "env": eye (1.8, -1.5, 1.0)
from env 0's origin, looking at its table):
  frame_ms      device-event time per render_rgb() (pose pass + render launch; median and spread over --rounds windows of
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
    ap.add_argument("--preroll", type=int, default=100)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lift_viewer_bench needs the GPU")
    from isaac_rover_orbit_amd.cfg import ViewerCfg
    from isaac_rover_orbit_amd.envs.lift_env import FrankaCubeLiftEnv, LiftEnvCfg

    n = a.envs
    cfg = LiftEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    env = FrankaCubeLiftEnv(cfg, render_mode="rgb_array")
    g = torch.Generator(device="cuda:0").manual_seed(0)
    env.reset()
    for _ in range(a.preroll):
        env.step(torch.rand(n, 8, device="cuda:0", generator=g) * 2 - 1)
    modes = {"world": ViewerCfg(eye=(-6.0, -6.0, 3.5), lookat=(0.0, 0.0, 0.0)),
             "env": ViewerCfg(eye=(1.8, -1.5, 1.0), lookat=(0.4, 0.0, 0.3), origin_type="env", env_index=0)}
    res = {"envs": n, "pixels": [1280, 720], "env_spacing": cfg.scene.env_spacing}
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
        torch.cuda.synchronize()
        overflow = int(env._viewer_ws[:1].view(torch.int32).item())          # the workspace's first word: envs on the overflow list
        med = statistics.median(ms)
        res[name] = {"frame_ms": round(med, 4), "frame_ms_rounds": [round(x, 4) for x in ms],
                     "grays_per_s": round(1280 * 720 / (med * 1e-3) / 1e9, 3), "host_ms": round(statistics.median(host), 3),
                     "env_pixels": int((ids >= 2).sum()), "envs_visible": int(torch.unique((ids[ids >= 2] - 2) // 16).numel()),
                     "overflow_envs": overflow}
    if a.trace_only:
        res["trace_renders_per_mode"] = a.renders
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
