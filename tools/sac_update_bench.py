#!/usr/bin/env python3
"""Times the SAC update, torch spec (isaac_rover_orbit_amd.sac.TorchSAC, float32 on the GPU) against the fused HIP update
(FusedSAC), at the reference's batch: 4096 rows drawn from a 16-slot, 4096-env replay memory of seeded synthetic transitions.

    python tools/sac_update_bench.py [--reps 5] [--steps 50] [--out profiles/sac_update_bench.json] [--fused-only]

Per item: device-synchronised wall clock over --steps back-to-back calls after a warm-up, divided by --steps, the two paths
alternated in one process (median, min, max over --reps rounds): one critic step, one policy step (with the entropy step) and
one whole update (critic, policy, Polyak).  The torch
items include the spec's ``memory.gather`` of the batch, as the fused items include their gather kernel.  --fused-only runs
the fused update alone (for a rocprofv3 --kernel-trace --stats run of its kernels)."""
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
from ppo_reference import load_example  # noqa: E402


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def summary(xs):
    return {"median_ms": 1e3 * statistics.median(xs), "min_ms": 1e3 * min(xs), "max_ms": 1e3 * max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from isaac_rover_orbit_amd.sac import FusedSAC, TorchSAC
    from isaac_rover_orbit_amd.td3 import Critic, ReplayMemory
    ex = load_example()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    pol, c1, c2 = ex.Net(2, True).to(dev), Critic().to(dev), Critic().to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    mem = ReplayMemory(args.slots, args.envs, device=dev)
    mem.obs.copy_(torch.randn(mem.obs.shape, device=dev, generator=g) * 0.5)
    mem.actions.copy_(torch.rand(mem.actions.shape, device=dev, generator=g) * 2 - 1)
    mem.rewards.copy_(torch.randn(mem.rewards.shape, device=dev, generator=g))
    mem.terminated.copy_(torch.rand(mem.terminated.shape, device=dev, generator=g) < 0.1)
    mem.ring_pos.copy_(torch.arange(args.slots, dtype=torch.int32, device=dev))
    mem.filled, mem.memory_index, mem.cursor = True, 0, args.slots
    B = args.batch
    idx = mem.sample_indices(B, g)
    eps = torch.randn(B, 4, device=dev, generator=g)
    fused = FusedSAC(pol.state_dict(), c1.state_dict(), c2.state_dict())
    spec = TorchSAC(pol, c1, c2)

    def t_critic():
        s, a, r, s2, t = mem.gather(idx)
        spec.critic_step(s, a, r, s2, t, eps[:, 0:2])

    def t_policy():
        spec.policy_step(mem.gather(idx)[0], eps[:, 2:4])

    items = [("fused_critic_step", lambda: fused.critic_step(mem, idx, eps)), ("fused_policy_step", lambda: fused.policy_step(mem, idx, eps)),
             ("fused_update", lambda: fused.update(mem, idx, eps))]
    if not args.fused_only:
        items += [("torch_critic_step", t_critic), ("torch_policy_step", t_policy), ("torch_update", lambda: spec.update(mem, idx, eps))]
    res = {k: [] for k, _ in items}
    for _ in range(3):                          # warm-up
        for _, fn in items:
            fn()
    for _ in range(args.reps):
        for k, fn in items:
            res[k].append(timed(fn, args.steps))
    st = fused.stats()
    out = {"rows": B, "memory_slots": args.slots, "envs": args.envs, "reps": args.reps, "steps": args.steps, "device": torch.cuda.get_device_name(0),
           **{k: summary(v) for k, v in res.items()},
           "fused_stats": {k: st[k] for k in ("critic_step", "actor_step", "entropy_step", "bad_index", "critic_loss", "policy_loss", "alpha")}}
    if not args.fused_only:
        out["fused_over_torch"] = {k: statistics.median(res["fused_" + k]) / statistics.median(res["torch_" + k])
                                   for k in ("critic_step", "policy_step", "update")}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
