#!/usr/bin/env python3
"""Times the fused DAgger path (isaac_rover_orbit_amd.dagger) on the GPU, beside FusedTD3's full update in the same run.

    python tools/dagger_bench.py [--reps 7] [--steps 30] [--out profiles/dagger_bench.json] [--no-env]

Items, alternated in one process; per item a host clock around --steps back-to-back calls that ends in a device synchronise, divided by
--steps; median, min and max over --reps rounds after a warm-up:

  dagger_update        one FusedDAgger.update at --batch rows drawn from a --slots x --envs memory of seeded synthetic rows and labels
  td3_update           one FusedTD3 update at the same batch on the same memory with policy_delay 1: critic step, actor step, Polyak.
                       The comparison of record: DAgger's update is one actor forward / backward / Adam of the same network, TD3's
                       holds that plus two critics
  torch_dagger_update  the float32 torch specification on the same device (with its memory.gather), for scale
  render_31x31         RoverEnv.render_depth() of --envs envs with dagger.student_camera_cfg() (reported, not targeted)
  collect              DAggerCollector.record + act on --envs envs: rows, teacher, student, mix, label, bookkeeping, indices
  collector_step       render_31x31 + collect
"""
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--no-env", action="store_true", help="the update items only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from isaac_rover_orbit_amd import dagger
    from isaac_rover_orbit_amd.policy import RoverNet
    from isaac_rover_orbit_amd.td3 import Critic, FusedTD3, ReplayMemory
    ex = load_example()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    student, teacher, actor, c1, c2 = ex.Net(2, True).to(dev), ex.Net(2, True).to(dev), ex.Net(2, False).to(dev), Critic().to(dev), Critic().to(dev)
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
    fused = dagger.FusedDAgger(student.state_dict())
    spec = dagger.TorchDAgger(student)
    td3 = FusedTD3(actor.state_dict(), c1.state_dict(), c2.state_dict(), policy_delay=1)
    items = [("dagger_update", lambda: fused.update(mem, idx)), ("td3_update", lambda: td3.update(mem, idx)),
             ("torch_dagger_update", lambda: spec.update(mem, idx))]
    env = None
    if not args.no_env:
        from isaac_rover_orbit_amd import terrain as T
        from isaac_rover_orbit_amd.cfg import RoverEnvCfg
        from isaac_rover_orbit_amd.envs import RoverEnv
        terrain = T.make_procedural_terrain((2048, 2048), seed=1234)
        terrain.make_spawns(2 * args.envs)
        cfg = RoverEnvCfg(); cfg.scene.num_envs = args.envs; cfg.terrain.kind = "custom"; cfg.camera = dagger.student_camera_cfg()
        env = RoverEnv(cfg, terrain=terrain)
        obs, _ = env.reset()
        obs, rew, term, _, _ = env.step(torch.zeros(args.envs, 2, device=dev))
        rows, depth = obs["policy"].clone(), env.render_depth()
        cmem = ReplayMemory(args.slots, args.envs, device=dev)
        col = dagger.DAggerCollector(RoverNet.from_state_dict(teacher.state_dict(), final_act="tanh"), fused.actor, cmem)
        col.begin(rows, depth)

        def collect():
            col.act(0.5)
            col.record(rows, depth, rew, term, B)

        def collector_step():
            d = env.render_depth()
            col.act(0.5)
            col.record(rows, d, rew, term, B)

        items += [("render_31x31", env.render_depth), ("collect", collect), ("collector_step", collector_step)]
    res = {k: [] for k, _ in items}
    for _ in range(3):                          # warm-up
        for _, fn in items:
            fn()
    for _ in range(args.reps):
        for k, fn in items:
            res[k].append(timed(fn, args.steps))
    st = fused.stats()
    out = {"rows": B, "memory_slots": args.slots, "envs": args.envs, "reps": args.reps, "steps": args.steps,
           "device": torch.cuda.get_device_name(0), **{k: summary(v) for k, v in res.items()},
           "dagger_over_td3_update": statistics.median(res["dagger_update"]) / statistics.median(res["td3_update"]),
           "dagger_over_torch_update": statistics.median(res["dagger_update"]) / statistics.median(res["torch_dagger_update"]),
           "dagger_stats": {k: st[k] for k in ("steps", "bad_index", "loss", "grad_norm")}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if env is not None:
        env.close()


if __name__ == "__main__":
    main()
