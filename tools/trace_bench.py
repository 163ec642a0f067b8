#!/usr/bin/env python3
"""Collection-loop throughput with the host recorder (trace.EpisodeRecorder) and the fused one (trace_collect.TraceCollector) at
the same settings, and the per-step time of the fused recorder's two kernels.

    python tools/trace_bench.py --envs 1024 --steps 128
    python tools/trace_bench.py --envs 256 --steps 48 --depth
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/trace_bench.py --envs 1024 --kernels-only   # per-kernel times

The loop is the one of examples/08_collect_traces.py: zero agent, ``env.step``, ``recorder.append``.  It is timed with a host clock
around work that ends in a device synchronise; ``close()`` (the same writer and the same compression for both recorders) is timed
separately.  The two recorders alternate, ``--reps`` times each.  The kernel figures come from device events around a batch of
appends without the env: the append + commit pair, and the commit kernel alone (``rover_trace_commit_all`` on an idle state: the
same kernel walking the same envs); their difference is the append kernel.  One JSON line per case goes to stdout.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isaac_rover_orbit_amd import terrain as T  # noqa: E402
from isaac_rover_orbit_amd.cfg import CameraCfg, RoverEnvCfg  # noqa: E402
from isaac_rover_orbit_amd.envs import RoverEnv  # noqa: E402
from isaac_rover_orbit_amd.trace import EpisodeRecorder  # noqa: E402
from isaac_rover_orbit_amd.trace_collect import TraceCollector  # noqa: E402

DEPTH = {"depth": {"shape": (160, 90), "dtype": np.float32}}


def make_env(args):
    ter = T.make_procedural_terrain((1024, 1024), seed=7, n_rocks=120)
    ter.make_spawns(2 * max(args.envs, 2048))
    cfg = RoverEnvCfg()
    cfg.scene.num_envs, cfg.sim.device, cfg.terrain.kind = args.envs, "cuda:0", "custom"
    cfg.episode_length_s = args.episode_steps * cfg.sim.dt * cfg.decimation      # time-outs inside the window
    cfg.camera = CameraCfg() if args.depth else None
    return RoverEnv(cfg, terrain=ter)


def loop(env, rec, steps, fused):
    """``steps`` steps of the collection loop; returns (loop seconds, close seconds, rows written)."""
    obs, info = env.reset()
    actions = torch.zeros(env.num_envs, 2, device="cuda:0")
    add = rec.append if fused else rec.append_to_buffer
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        nxt, rew, terminated, truncated, nxt_info = env.step(actions)
        add(obs["policy"], actions, rew, terminated | truncated, info)
        obs, info = nxt, nxt_info
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    rec.close()
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, steps * env.num_envs


def kernel_times(args, extras, batch=50):
    """Device-event time per step of append + commit, and of the commit kernel alone, in microseconds."""
    n, tmp = args.envs, tempfile.mkdtemp(prefix="trace_bench_")
    batch = max(1, min(batch, args.episode_steps - 1))     # the batch and the closing row fit one episode
    col = TraceCollector(os.path.join(tmp, "k"), n, 965, 2, extras, max_episode_rows=args.episode_steps, drain_interval=batch + 2)
    obs, act, rew = torch.randn(n, 965, device="cuda:0"), torch.zeros(n, 2, device="cuda:0"), torch.randn(n, device="cuda:0")
    done = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    info = {"depth": torch.randn(n, 90, 160, device="cuda:0").permute(0, 2, 1)} if extras else None
    out = {}
    for name in ("warm", "pair"):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(batch):
            col.append(obs, act, rew, done, info)
        ev[1].record()
        torch.cuda.synchronize()
        out[name] = ev[0].elapsed_time(ev[1]) * 1e3 / batch
        done.fill_(True)
        col.append(obs, act, rew, done, info)          # every episode ends; the drain empties the rings
        col.drain()
        done.fill_(False)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(batch):
        col._commit_all()
    ev[1].record()
    torch.cuda.synchronize()
    commit = ev[0].elapsed_time(ev[1]) * 1e3 / batch
    col.close()
    shutil.rmtree(tmp, ignore_errors=True)
    return {"append_commit_us": round(out["pair"], 2), "commit_us": round(commit, 2), "append_us": round(out["pair"] - commit, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--episode-steps", type=int, default=50, help="env time-out in steps (= max_episode_rows)")
    ap.add_argument("--drain-interval", type=int, default=64)
    ap.add_argument("--depth", action="store_true", help="RoverEnv with the depth camera; extras['depth'] is recorded")
    ap.add_argument("--kernels-only", action="store_true", help="only the fused recorder's kernels, without the env")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trace_bench.py measures on a ROCm GPU; none is available")
    extras = DEPTH if args.depth else None
    res = {"envs": args.envs, "steps": args.steps, "depth": bool(args.depth), "episode_steps": args.episode_steps,
           "drain_interval": args.drain_interval, "device_bytes": TraceCollector.device_bytes(args.envs, 965, 2, extras, args.episode_steps,
                                                                                             args.drain_interval)}
    res.update(kernel_times(args, extras))
    if not args.kernels_only:
        env = make_env(args)
        tmp = tempfile.mkdtemp(prefix="trace_bench_")

        def recorder(fused, tag):
            base = os.path.join(tmp, tag)
            if fused:
                return TraceCollector(base, args.envs, 965, 2, extras, env=env, drain_interval=args.drain_interval)
            return EpisodeRecorder(base, args.envs, 965, 2, extras)
        for fused in (False, True):
            loop(env, recorder(fused, f"warm{int(fused)}"), args.warmup, fused)
        runs = {False: [], True: []}
        for r in range(args.reps):
            for fused in (False, True):
                runs[fused].append(loop(env, recorder(fused, f"r{r}_{int(fused)}"), args.steps, fused))
            shutil.rmtree(tmp, ignore_errors=True)
            os.makedirs(tmp, exist_ok=True)
        for fused, name in ((False, "host"), (True, "fused")):
            best = min(runs[fused], key=lambda x: x[0])
            res[f"{name}_loop_steps_per_s"] = round(args.steps / best[0], 2)
            res[f"{name}_loop_s_all"] = [round(x[0], 4) for x in runs[fused]]
            res[f"{name}_close_s_all"] = [round(x[1], 3) for x in runs[fused]]
            res[f"{name}_total_steps_per_s"] = round(args.steps / min(x[0] + x[1] for x in runs[fused]), 3)
        res["loop_speedup"] = round(res["fused_loop_steps_per_s"] / res["host_loop_steps_per_s"], 2)
        env.close()
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
