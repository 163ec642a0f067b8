#!/usr/bin/env python3
"""Times one TD3 gradient step, torch spec (isaac_rover_orbit_amd.td3.TorchTD3) against the fused HIP update (FusedTD3), at
the reference's shapes: batch 4096 sampled from a replay memory of 4096 envs, on seeded synthetic transitions.

    python tools/td3_update_bench.py [--reps 50] [--out profiles/td3_update_bench.json] [--fused-only]

Per item: device-synchronised wall clock of --reps steps after a warm-up, the two paths alternated in one process (median,
min, max of the per-step time over 5 rounds): a critic step alone, and a critic + actor + Polyak step (the policy-delay
step).  Both paths read the same index batches.  --fused-only runs the fused step alone (for a rocprofv3 --kernel-trace
--stats run of its kernels)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from td3_helpers import fill, nets  # noqa: E402


def summary(xs):
    return {"median_ms": 1e3 * statistics.median(xs), "min_ms": 1e3 * min(xs), "max_ms": 1e3 * max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--memory", type=int, default=16, help="memory slots (the reference uses 2 x batch = 8192)")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from isaac_rover_orbit_amd.td3 import FusedTD3, ReplayMemory, TorchTD3
    dev = torch.device("cuda")
    pol, c1, c2 = nets(0, dev)
    mem = ReplayMemory(args.memory, args.envs, device=dev)
    fill(mem, args.memory + 1)
    g = torch.Generator(device=dev).manual_seed(1)
    idxs = [mem.sample_indices(args.batch, g) for _ in range(args.reps)]
    fused = FusedTD3(pol.state_dict(), c1.state_dict(), c2.state_dict())
    spec = TorchTD3(pol, c1, c2)

    def f_critic():
        for idx in idxs:
            fused.critic_step(mem, idx)

    def f_full():
        for idx in idxs:
            fused.critic_step(mem, idx)
            fused.actor_step(mem, idx)
            fused.polyak()

    def t_critic():
        for idx in idxs:
            spec.critic_step(*mem.gather(idx))

    def t_full():
        for idx in idxs:
            s, a, r, s2, t = mem.gather(idx)
            spec.critic_step(s, a, r, s2, t)
            spec.actor_step(s)
            spec.polyak()

    items = [("fused_critic_step", f_critic), ("fused_critic_actor_polyak", f_full)]
    if not args.fused_only:
        items += [("torch_critic_step", t_critic), ("torch_critic_actor_polyak", t_full)]
    for _, fn in items:                         # warm-up
        fn()
    res = {k: [] for k, _ in items}
    for _ in range(args.rounds):
        for k, fn in items:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            res[k].append((time.perf_counter() - t0) / len(idxs))
    out = {"batch": args.batch, "envs": args.envs, "memory_slots": args.memory, "steps_per_round": len(idxs), "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), **{k: summary(v) for k, v in res.items()}}
    if not args.fused_only:
        for k in ("critic_step", "critic_actor_polyak"):
            out[f"speedup_{k}"] = out[f"torch_{k}"]["median_ms"] / out[f"fused_{k}"]["median_ms"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
