#!/usr/bin/env python3
"""Times the lift task's PPO update: the torch spec (isaac_rover_orbit_amd.lift_ppo.TorchLiftPPO) against the fused HIP update
(FusedLiftPPO) at the skrl_ppo_cfg.yaml shapes: 4096 envs x 24 rollouts, 8 epochs x 24 minibatches of 4096 rows, on seeded
synthetic buffers whose KL stays below the early-stop threshold (every minibatch steps).

    python tools/lift_ppo_bench.py [--reps 20] [--out profiles/lift_ppo_update_bench.json] [--fused-only]

Per item: device-synchronised wall clock after warm-up, the two paths alternated in one process (median, min, max over --reps).
--fused-only runs the fused update alone (for a rocprofv3 --kernel-trace --stats run of its kernels)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isaac_rover_orbit_amd import lift_ppo as LP  # noqa: E402


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
    ap.add_argument("--rollouts", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--update-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fused-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    pol, val = LP.LiftMLP(8, log_std=True).to(dev), LP.LiftMLP(1).to(dev)
    B = args.envs * args.rollouts
    g = torch.Generator(device=dev).manual_seed(1)
    obs = torch.randn(B, 36, device=dev, generator=g)
    with torch.no_grad():
        mean = torch.cat([pol(obs[i:i + 65536]) for i in range(0, B, 65536)])
        v0 = torch.cat([val(obs[i:i + 65536])[:, 0] for i in range(0, B, 65536)])
        act = (mean + torch.randn(B, 8, device=dev, generator=g)).contiguous()
        logp = LP.gaussian_logp(mean, pol.log_std_parameter, act).contiguous()
    oldv = (v0 + 0.3 * torch.randn(B, device=dev, generator=g)).contiguous()
    ret = (oldv + torch.randn(B, device=dev, generator=g)).contiguous()
    adv = torch.randn(B, device=dev, generator=g)
    data = (obs, act, logp, oldv, ret, adv)
    mbs = 24
    perms = [torch.randperm(B, device=dev) for _ in range(8)]
    n_mb = B // mbs
    idx = perms[0][:n_mb].contiguous()

    fused = LP.FusedLiftPPO(pol.state_dict(), val.state_dict(), kl_early_stop=0.0)
    spec = LP.TorchLiftPPO(LP.LiftMLP(8, log_std=True).to(dev), LP.LiftMLP(1).to(dev), kl_early_stop=0.0)
    spec.policy.load_state_dict(pol.state_dict()); spec.value.load_state_dict(val.state_dict())
    params = list(spec.policy.parameters()) + list(spec.value.parameters())

    def mb_fused():
        fused.minibatch(*data, idx)
        fused.apply()

    def mb_torch():
        s = spec.state_preprocessor(obs[idx])
        loss, kl, _, _ = LP.lift_ppo_loss(spec.policy, spec.value, s, act[idx], logp[idx], oldv[idx], ret[idx], adv[idx])
        spec.opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        spec.opt.step()

    res = {"envs": args.envs, "rollouts": args.rollouts, "minibatch_rows": n_mb, "epochs": 8, "minibatches": mbs,
           "device": torch.cuda.get_device_name(0)}
    for _ in range(5):
        mb_fused()
        if not args.fused_only:
            mb_torch()
    tf, tt = [], []
    for _ in range(args.reps):
        tf.append(timed(mb_fused))
        if not args.fused_only:
            tt.append(timed(mb_torch))
    res["minibatch_fused"] = summary(tf)
    if tt:
        res["minibatch_torch"] = summary(tt)
    uf, ut = [], []
    for _ in range(args.update_reps):
        uf.append(timed(lambda: fused.update(*data, perms=perms)))
        if not args.fused_only:
            ut.append(timed(lambda: spec.update(*data, perms=perms)))
    res["update_fused"] = summary(uf)
    if ut:
        res["update_torch"] = summary(ut)
        res["update_speedup"] = res["update_torch"]["median_ms"] / res["update_fused"]["median_ms"]
    flop = 0
    for k, n in ((36, 256), (256, 128), (128, 64)):
        flop += 2 * 2 * n_mb * k * n * 3          # both networks, forward + dA + dW
    flop += 2 * n_mb * 64 * 9 * 3
    res["minibatch_model"] = {"gflop": flop / 1e9, "tflops_at_median": flop / (res["minibatch_fused"]["median_ms"] * 1e-3) / 1e12}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
