#!/usr/bin/env python3
"""Collect episode traces into the reference's recorder layout (counterpart of the reference's SequentialCollectorOrbit.collect,
rover_envs/utils/recorder/orbit.py:23-34, with HDF5DataRecorder): predict, step, append, until enough episodes are on disk.

    python examples/08_collect_traces.py --out traces/run --envs 1024 --episodes 4096                 # zero agent, fused recorder
    python examples/08_collect_traces.py --out traces/run --envs 256 --episodes 512 --depth            # + extras["depth"]
    python examples/08_collect_traces.py --out traces/run --checkpoint <.../best_agent.pt> --recorder host

``--recorder fused`` (default) keeps the rows on the device (isaac_rover_orbit_amd.trace_collect.TraceCollector: two launches per
step, one synchronisation per drain); ``--recorder host`` is trace.EpisodeRecorder, which copies every tensor to the host each
step.  Both write the same files.  Unlike the reference's loop, which resets EVERY env as soon as any env is done, resets are
left to the env: each env starts its next episode on its own, as everywhere else in this project.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isaac_rover_orbit_amd import terrain as T  # noqa: E402
from isaac_rover_orbit_amd.cfg import CameraCfg, RoverEnvCfg  # noqa: E402
from isaac_rover_orbit_amd.envs import RoverEnv  # noqa: E402
from isaac_rover_orbit_amd.trace import EpisodeRecorder, load_trace  # noqa: E402
from isaac_rover_orbit_amd.trace_collect import TraceCollector  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="traces/run", help="base file name, without extension")
    ap.add_argument("--recorder", choices=("host", "fused"), default="fused")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--episodes", type=int, default=1024, help="stop once this many episodes have ended")
    ap.add_argument("--depth", action="store_true", help="RoverEnv with the depth camera; extras['depth'] is recorded")
    ap.add_argument("--checkpoint", default=None, help="skrl checkpoint of the actor; default: the zero agent")
    ap.add_argument("--episode_length_s", type=float, default=None)
    ap.add_argument("--max_rows", type=int, default=500_000)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    terrain = T.make_procedural_terrain((2048, 2048), seed=1234)
    terrain.make_spawns(2 * args.envs)
    cfg = RoverEnvCfg()
    cfg.scene.num_envs, cfg.terrain.kind = args.envs, "custom"
    cfg.camera = CameraCfg() if args.depth else None
    if args.episode_length_s is not None:
        cfg.episode_length_s = args.episode_length_s
    env = RoverEnv(cfg, terrain=terrain)
    device = env.unwrapped.device
    extras = {"depth": {"shape": (160, 90), "dtype": np.float32}} if args.depth else None
    if args.checkpoint:
        from isaac_rover_orbit_amd.policy import RoverNet
        actor = RoverNet.from_checkpoint(args.checkpoint, role="policy")
        predict_fn = lambda obs: actor.act({"policy": torch.nan_to_num(obs["policy"], neginf=0.0)})   # noqa: E731
    else:
        zeros = torch.zeros(args.envs, 2, device=device)
        predict_fn = lambda obs: zeros   # noqa: E731
    if args.recorder == "fused":
        print(f"device memory of the recorder: {TraceCollector.device_bytes(args.envs, 965, 2, extras, env.max_episode_length) / 2**30:.2f} GiB")
        rec = TraceCollector(args.out, args.envs, 965, 2, extras, max_rows=args.max_rows, env=env, device=device)
        append = rec.append
    else:
        rec = EpisodeRecorder(args.out, args.envs, 965, 2, extras, max_rows=args.max_rows)
        append = rec.append_to_buffer
    finished = torch.zeros((), dtype=torch.int64, device=device)
    obs, info = env.reset()
    steps, t0 = 0, time.perf_counter()
    with torch.no_grad():
        while True:
            action = predict_fn(obs)
            next_obs, reward, terminated, truncated, next_info = env.step(action)
            done = terminated | truncated
            append(obs["policy"], action, reward, done, info)
            finished += done.sum()
            obs, info, steps = next_obs, next_info, steps + 1
            if steps % 64 == 0 and int(finished) >= args.episodes:     # one read-back per 64 steps
                break
    files = rec.close()
    dt = time.perf_counter() - t0
    rows = sum(load_trace(f)["number_of_steps"] for f in files)
    print(f"{steps} steps x {args.envs} envs in {dt:.1f} s ({steps / dt:.1f} steps/s, close included); {int(finished)} episodes ended; "
          f"{rows} rows in {len(files)} file(s): {files[0]} ...")
    env.close()


if __name__ == "__main__":
    main()
