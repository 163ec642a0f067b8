#!/usr/bin/env python3
"""Times the TRPO update, torch spec (isaac_rover_orbit_amd.trpo.TorchTRPO) against the fused HIP update (FusedTRPO), at the
reference's shapes: 4096 envs x 60 rollouts (245 760 rows), value regression 4 epochs x 60 minibatches of 4096 rows, on
seeded synthetic buffers.

    python tools/trpo_update_bench.py [--reps 5] [--out profiles/trpo_update_bench.json] [--fused-only]

Per item: device-synchronised wall clock after one warm-up, the two paths alternated in one process (median, min, max over
--reps): one policy step (gradient, CG, step, line search), one value pass (240 minibatches + Adam steps) and one whole
update.  Every policy step starts from the same parameters.  --fused-only runs the fused update alone (for a rocprofv3
--kernel-trace --stats run of its kernels)."""
import argparse
import copy
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(xs):
    return {"median_ms": 1e3 * statistics.median(xs), "min_ms": 1e3 * min(xs), "max_ms": 1e3 * max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rollouts", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from isaac_rover_orbit_amd.trpo import FusedTRPO, TorchTRPO
    ex = load_example()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    pol, val = ex.Net(2, True).to(dev), ex.Net(1, False).to(dev)
    B = args.envs * args.rollouts
    g = torch.Generator(device=dev).manual_seed(1)
    obs = torch.randn(B, 965, device=dev, generator=g) * 0.5
    with torch.no_grad():
        mean = torch.cat([pol(obs[i:i + 8192]) for i in range(0, B, 8192)])
        act = (mean + torch.randn(B, 2, device=dev, generator=g)).contiguous()
        logp = ((-0.5 * (act - mean) ** 2 - 0.9189385332).sum(1) + 0.05 * torch.randn(B, device=dev, generator=g)).contiguous()
    adv = torch.randn(B, device=dev, generator=g)
    adv = ((adv - adv.mean()) / (adv.std() + 1e-8)).contiguous()
    ret = torch.randn(B, device=dev, generator=g)
    perms = [torch.randperm(B, device=dev) for _ in range(4)]
    sd_p, sd_v = copy.deepcopy(pol.state_dict()), copy.deepcopy(val.state_dict())

    fused = FusedTRPO(sd_p, sd_v)
    p0 = fused.params.clone()

    def f_policy():
        fused.params.copy_(p0)
        fused.policy_step(obs, act, logp, adv)

    def f_value():
        for perm in perms:
            for mb in perm.chunk(60):
                fused.value_minibatch(obs, ret, mb.contiguous())
                fused.value_apply()

    def f_update():
        fused.params.copy_(p0)
        fused.update(obs, act, logp, ret, adv, perms=perms)

    spec = TorchTRPO(pol, val)

    def t_policy():
        pol.load_state_dict(sd_p)
        spec.policy_step(obs, act, logp, adv)

    def t_value():
        spec.value_pass(obs, ret, perms)

    def t_update():
        pol.load_state_dict(sd_p)
        spec.update(obs, act, logp, ret, adv, perms=perms)

    items = [("fused_policy_step", f_policy), ("fused_value_pass", f_value), ("fused_update", f_update)]
    if not args.fused_only:
        items += [("torch_policy_step", t_policy), ("torch_value_pass", t_value), ("torch_update", t_update)]
    res = {k: [] for k, _ in items}
    for _, fn in items:                         # warm-up
        fn()
    for _ in range(args.reps):
        for k, fn in items:
            res[k].append(timed(fn))
    f_policy()
    st = fused.stats()
    out = {"rows": B, "value_minibatch_rows": B // 60, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           **{k: summary(v) for k, v in res.items()},
           "fused_policy_step_stats": {k: st[k] for k in ("cg_iters", "rr", "xhx", "step", "accepted", "trials", "kl")}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
