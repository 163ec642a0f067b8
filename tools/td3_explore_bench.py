#!/usr/bin/env python3
"""Times rover_td3_explore_act in each mode against rover_td3_collect_act at 4096 rows (the reference's env count), on random packed
weights and seeded synthetic rows.

    python tools/td3_explore_bench.py [--rows 4096] [--rounds 20] [--launches 200] [--parent-lib PATH] [--out profiles/td3_explore_bench.json]

Per item and round: device events around --launches back-to-back launches on one stream, after a warm-up of every item; the items
are alternated inside each round, all in one process.  The figure of an item is the mean over rounds of the per-launch time, with
the smallest and largest round beside it (the run-to-run spread).  --parent-lib names a librover_hip.so built from the parent
commit: its rover_td3_collect_act is then timed as a further item, in the same rounds."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import random_policy_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("td3_explore_bench needs a ROCm GPU: nothing is measured without one")
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd import td3_collect as TC
    from isaac_rover_orbit_amd import td3_explore as TE
    from isaac_rover_orbit_amd.policy import RoverNet
    dev = torch.device("cuda")
    ws, bs = random_policy_weights(seed=21, out_dim=2, scale=3.0)
    actor = RoverNet(ws, bs, n_enc=2, final_act="none")
    n = args.rows
    g = torch.Generator(device=dev).manual_seed(1)
    rows = (torch.randn(n, 965, device=dev, generator=g) * 0.5).contiguous()
    act, env_act, state = (torch.zeros(n, 2, device=dev) for _ in range(3))

    def explore(mode):
        hp = TE.default_hparams()
        hp.mode, hp.noise_std = mode, 0.1
        return lambda k: TE.explore_act(actor, rows, k, hp, act, env_act, ou_state=state if mode == TE.OU else None)

    chp = TC.default_hparams()
    chp.explore, chp.noise_std = 1, 0.1
    items = [("collect_act_gaussian", lambda k: TC.collect_act(actor, rows, k, chp, act, env_act)),
             ("explore_off", explore(TE.OFF)), ("explore_gaussian", explore(TE.GAUSSIAN)), ("explore_ou", explore(TE.OU)),
             ("explore_random", explore(TE.RANDOM))]
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        parent.rover_td3_collect_act.argtypes = _lib.load().rover_td3_collect_act.argtypes
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def parent_act(k):
            rc = parent.rover_td3_collect_act(C.byref(actor.desc), actor.packed.data_ptr(), actor.n_copies, C.byref(chp), C.c_uint64(k),
                                              rows.data_ptr(), n, None, act.data_ptr(), env_act.data_ptr(), None, stream)
            if rc != 0:
                sys.exit(f"the parent library's rover_td3_collect_act failed (code {rc})")
        items.insert(0, ("parent_collect_act_gaussian", parent_act))
    for _, fn in items:                         # warm-up: code objects, the LDS attribute
        for k in range(10):
            fn(k)
    torch.cuda.synchronize()
    res = {name: [] for name, _ in items}
    for r in range(args.rounds):
        for name, fn in items:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(args.launches):
                fn(r * args.launches + k)
            e1.record()
            e1.synchronize()
            res[name].append(1e3 * e0.elapsed_time(e1) / args.launches)
    out = {"rows": n, "rounds": args.rounds, "launches_per_round": args.launches, "device": torch.cuda.get_device_name(0),
           "unit": "us per launch, device events around back-to-back launches",
           **{k: {"mean_us": statistics.fmean(v), "min_us": min(v), "max_us": max(v)} for k, v in res.items()}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
