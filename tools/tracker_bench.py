#!/usr/bin/env python3
"""Dev tool (GPU box): what skrl's reward / episode tracking costs per env step at the reference's size (4096 envs), without the env.

Three forms on the same seeded rewards and flags (about 1 % of the envs finish per step), alternated in one process over windows
that end in a device synchronise (host clock); the median and the spread over the windows are reported:

  fused     tracker.EpisodeTracker.step + .track_vector with a 16-float device vector: three launches, no synchronisation
  skrl      tracker.SkrlTracking.record_transition on the same device tensors + the reference trainer's 13 ``v.item()`` on a device
            log vector (skrl_utils.py:139-142): what skrl's way costs, its host synchronisations included
  snapshot  one EpisodeTracker write (one launch, one device-to-host copy, the dict): once per write interval, not per step

Host synchronisations between writes and launches per step are counted, not timed: the fused form's are fixed by construction
(0 and 3), skrl's synchronisations are counted by what it calls per step.

    python tools/tracker_bench.py [--rounds 5] [--out profiles/tracker_bench.json]
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
from isaac_rover_orbit_amd import tracker as T  # noqa: E402


def windows(forms, rounds):
    """forms: {name: (fn, calls per window)}.  Alternates the forms; returns {name: [seconds per call]}."""
    res = {k: [] for k in forms}
    for fn, _ in forms.values():                # warm every shape
        fn(); fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, (fn, calls) in forms.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            res[k].append((time.perf_counter() - t0) / calls)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4000, help="steps per window of the fused form (skrl: a fifth, snapshot: a tenth)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracker_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tracker_bench needs a ROCm GPU: nothing is measured without one")
    if args.rounds < 5:
        sys.exit("at least five windows per form")
    n, dev = args.num_envs, torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    S = 64                                       # distinct steps, cycled
    rew = torch.randn(S, n, device=dev, generator=g)
    term = (torch.rand(S, n, device=dev, generator=g) < 0.008).float()
    trunc = (torch.rand(S, n, device=dev, generator=g) < 0.002).float()
    logv = torch.randn(16, device=dev, generator=g)
    tags = tuple(f"EpisodeInfo / word {i}" for i in range(13))
    trk = T.EpisodeTracker(n, tags=tags, write_interval=40)
    sk = T.SkrlTracking(write_interval=0)
    k = {"fused": 0, "skrl": 0}

    def fused():
        i = k["fused"] = (k["fused"] + 1) % S
        trk.step(rew[i], term[i], trunc[i])
        trk.track_vector(tags, logv)

    def skrl():
        i = k["skrl"] = (k["skrl"] + 1) % S
        sk.record_transition(rew[i], term[i], trunc[i])
        for j, tag in enumerate(tags):           # skrl_utils.py:139-142: one .item() per infos["episode"] entry
            sk.track_data(tag, logv[j].item())
        if not k["skrl"]:                        # the lists are cleared as a write would clear them
            sk.tracking_data.clear()

    def snapshot():
        fused()
        trk.write(0)

    forms = {"fused": (fused, args.calls), "skrl": (skrl, max(args.calls // 5, 1)), "snapshot": (snapshot, max(args.calls // 10, 1))}
    res = windows(forms, args.rounds)
    out = {"num_envs": n, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per call, host clock around a "
           "window that ends in a device synchronise", "calls_per_window": {k_: c for k_, (_, c) in forms.items()}}
    for name, v in res.items():
        us = [x * 1e6 for x in v]
        out[name] = {"median": statistics.median(us), "min": min(us), "max": max(us), "windows": us}
        print(f"  {name:9s} median {out[name]['median']:9.2f} us  min {min(us):9.2f}  max {max(us):9.2f}", flush=True)
    out["snapshot_alone"] = out["snapshot"]["median"] - out["fused"]["median"]
    out["by_construction"] = {"fused_host_synchronisations_between_writes": 0, "fused_launches_per_step": 3,
                              "skrl_host_synchronisations_per_step": "nonzero + 2 tolist (when an env finished) + 3 item + 13 item"}
    spread = (out["fused"]["max"] - out["fused"]["min"]) + (out["skrl"]["max"] - out["skrl"]["min"])
    diff = out["skrl"]["median"] - out["fused"]["median"]
    out["skrl_minus_fused"] = {"us": diff, "spreads_together": spread, "exceeds_spreads": abs(diff) > spread}
    print(f"  skrl - fused = {diff:.2f} us; the two spreads together {spread:.2f} us", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
