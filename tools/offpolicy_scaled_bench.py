#!/usr/bin/env python3
"""Dev tool (GPU box): what skrl's running state scaler costs a TD3 / SAC gradient step at the reference's batch (4096 rows out of a
memory of ``--slots`` x ``--num_envs`` rows), and what the two staging kernels take alone.

Every form runs in one process, alternated over windows that end in a device synchronise (host clock); the median and the spread over
the windows are reported:

  update  -- one gradient step on the same sample:
               td3_plain   td3.FusedTD3.update                        (the yardstick: unchanged code)
               td3_scaled  offpolicy_scaled.FusedScaledTD3.update     (resolve, 2 x scaler train, 2 x stage rows, the same update)
               sac_plain   sac.FusedSAC.update
               sac_scaled  offpolicy_scaled.FusedScaledSAC.update
  kernels -- one launch each:
               resolve     rover_offpolicy_stage_resolve over the batch
               stage       rover_offpolicy_stage_rows of the batch's s rows out of the ring (random rows: source and destination
                           phases differ for three rows in four)
               apply_16B   rover_scaler_apply over a compact (batch, 965) image whose input and output share their alignment: its
                           16-byte path, the same bytes moved with no gather
               apply_4B    the same with the input one float off: rover_scaler_apply's element-by-element path, what an "only where
                           the phases agree" rule would do to three staged rows in four
               train       rover_scaler_train on the batch's ring rows (four launches)

    python tools/offpolicy_scaled_bench.py [--rounds 7] [--out profiles/offpolicy_scaled_bench.json]
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
from isaac_rover_orbit_amd import offpolicy_scaled as OS  # noqa: E402
from isaac_rover_orbit_amd.sac import FusedSAC  # noqa: E402
from isaac_rover_orbit_amd.scaler import DeviceScaler  # noqa: E402
from isaac_rover_orbit_amd.td3 import Critic, FusedTD3, ReplayMemory  # noqa: E402

OBS = 965


def load_example():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_ppo_example", os.path.join(ROOT, "examples", "04_train_ppo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


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


def summary(res, forms):
    out = {}
    for k, v in res.items():
        us = [x * 1e6 for x in v]
        out[k] = {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "calls_per_window": forms[k][1],
                  "windows_us": us}
        print(f"  {k:11s} median {out[k]['median_us']:10.2f} us  min {min(us):10.2f}  max {max(us):10.2f}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=64, help="memory slots (the ring holds one more): 64 x 4096 rows are 1 GB")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--update_calls", type=int, default=50)
    ap.add_argument("--kernel_calls", type=int, default=500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("offpolicy_scaled_bench needs a ROCm GPU: nothing is measured without one")
    if args.rounds < 5:
        sys.exit("at least five windows per form")
    dev = torch.device("cuda")
    ex = load_example()
    torch.manual_seed(42)
    g = torch.Generator(device=dev).manual_seed(1)
    M, N, B = args.slots, args.num_envs, args.batch
    mem = ReplayMemory(M, N, device=dev)
    col = torch.rand(OBS, device=dev, generator=g)
    for s in range(mem.slots):                  # rows of the rover's kind: columns of different scale and offset
        mem.obs[s] = torch.randn(N, OBS, device=dev, generator=g) * (0.2 + 4.0 * col) + (col - 0.5) * 6.0
    mem.actions.copy_(torch.rand(M, N, 2, device=dev, generator=g) * 2 - 1)
    mem.rewards.copy_(torch.randn(M, N, device=dev, generator=g))
    mem.terminated.copy_(torch.rand(M, N, device=dev, generator=g) < 0.05)
    mem.ring_pos.copy_(torch.arange(M, dtype=torch.int32, device=dev))
    mem.filled = True
    idx = torch.randint(0, len(mem), (B,), device=dev, generator=g)
    noise = torch.randn(B, 2, device=dev, generator=g) * 0.2
    eps = torch.randn(B, 4, device=dev, generator=g)

    c1, c2 = Critic().state_dict(), Critic().state_dict()
    td3_sd, sac_sd = ex.Net(2, False).state_dict(), ex.Net(2, True).state_dict()
    td3_plain, sac_plain = FusedTD3(td3_sd, c1, c2), FusedSAC(sac_sd, c1, c2)
    td3_scaled, sac_scaled = OS.FusedScaledTD3(FusedTD3(td3_sd, c1, c2)), OS.FusedScaledSAC(FusedSAC(sac_sd, c1, c2))
    print(f"[update, batch {B} of {len(mem)} rows, {args.rounds} alternated windows of {args.update_calls} steps] us per gradient step",
          flush=True)
    forms = {"td3_plain": (lambda: td3_plain.update(mem, idx, noise), args.update_calls),
             "td3_scaled": (lambda: td3_scaled.update(mem, idx, noise), args.update_calls),
             "sac_plain": (lambda: sac_plain.update(mem, idx, eps), args.update_calls),
             "sac_scaled": (lambda: sac_scaled.update(mem, idx, eps), args.update_calls)}
    update = summary(windows(forms, args.rounds), forms)

    sc = DeviceScaler(OBS, dev)
    staged, bad = OS.StagedBatch(B, dev), torch.zeros(1, dtype=torch.int32, device=dev)
    OS.stage_resolve(mem, idx, staged, bad)
    sc.train(mem.obs, staged.rows_s)
    image = torch.empty(B * OBS + 4, device=dev)
    aligned, off_by_one = image[:B * OBS].view(B, OBS), image[1:1 + B * OBS].view(B, OBS)
    out = torch.empty(B, OBS, device=dev)
    print(f"[kernels, {args.rounds} alternated windows of {args.kernel_calls} calls] us per call", flush=True)
    forms = {"resolve": (lambda: OS.stage_resolve(mem, idx, staged, bad), args.kernel_calls),
             "stage": (lambda: OS.stage_rows(sc, mem.obs, staged.rows_s, staged.obs[0]), args.kernel_calls),
             "apply_16B": (lambda: sc.forward(aligned, out=out), args.kernel_calls),
             "apply_4B": (lambda: sc.forward(off_by_one, out=out), args.kernel_calls),
             "train": (lambda: sc.train(mem.obs, staged.rows_s), args.kernel_calls)}
    kernels = summary(windows(forms, args.rounds), forms)
    moved = 2 * B * OBS * 4
    result = {"device": torch.cuda.get_device_name(0), "batch": B, "memory_rows": len(mem), "rounds": args.rounds,
              "update": update, "kernels": kernels,
              "scaled_over_plain": {a: update[a + "_scaled"]["median_us"] / update[a + "_plain"]["median_us"] for a in ("td3", "sac")},
              "scaled_minus_plain_us": {a: update[a + "_scaled"]["median_us"] - update[a + "_plain"]["median_us"] for a in ("td3", "sac")},
              "stage_bytes_moved": moved,
              "stage_gb_per_s": moved / kernels["stage"]["median_us"] / 1e3,
              "bad_index": int(bad.item()) | td3_scaled.stats()["bad_index"] | sac_scaled.stats()["bad_index"]}
    print(json.dumps({k: v for k, v in result.items() if k not in ("update", "kernels")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
