#!/usr/bin/env python3
"""Times the PPO update of examples/04_train_ppo.py against the fused HIP update (isaac_rover_orbit_amd.ppo.FusedPPO) at the
example's shapes: 4096 envs x 60 rollouts, 4 epochs x 60 minibatches of 4096 rows, on seeded synthetic buffers.

    python tools/ppo_update_bench.py [--reps 20] [--out profiles/ppo_update_bench.json] [--fused-only]

Per item: device-synchronised wall clock after warm-up, the two paths alternated in one process (median, min, max over
--reps).  --fused-only runs the fused update alone (for a rocprofv3 --kernel-trace --stats run of its kernels).

--gate times the gated update (include/rover_train_gate.h) instead, in one call, after warm-up, the four items alternated within
every repetition on the same permutations: the ungated update twice (their difference is the run-to-run spread), the gated update
with a threshold above every KL (every launch does its work behind the stop word's load), and the gated update with a threshold
below every KL (every epoch stops at its first minibatch: 59 skipped minibatches and 60 skipped applies per epoch, launch overhead
only)."""
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

SHAPES = [(80, 961), (60, 80), (256, 64), (160, 256), (128, 160)]


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--update-reps", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--gate", action="store_true", help="time the gated update against the ungated one (--gate-reps repetitions)")
    ap.add_argument("--gate-reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from isaac_rover_orbit_amd.ppo import FusedPPO
    ex = load_example()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    pol, val = ex.Net(2, True).to(dev), ex.Net(1, False).to(dev)
    n, T = args.envs, args.rollouts
    B = n * T
    g = torch.Generator(device=dev).manual_seed(1)
    obs = torch.randn(B, 965, device=dev, generator=g) * 0.5
    act = torch.randn(B, 2, device=dev, generator=g) * 0.5
    with torch.no_grad():
        ls = pol.log_std_parameter.clamp(-20.0, 2.0)
        mean = torch.cat([pol(obs[i:i + 16384]) for i in range(0, B, 16384)])
        logp = ((-0.5 * ((act - mean) / ls.exp()) ** 2 - ls - 0.9189385332).sum(1) + 0.1 * torch.randn(B, device=dev, generator=g))
        vals = torch.cat([val(obs[i:i + 16384])[:, 0] for i in range(0, B, 16384)])
    rew = torch.randn(T, n, device=dev, generator=g)
    done = (torch.rand(T, n, device=dev, generator=g) < 0.01).float()
    last_v = torch.randn(n, device=dev, generator=g)
    ret = vals + torch.randn(B, device=dev, generator=g)
    adv = torch.randn(B, device=dev, generator=g)
    fused = FusedPPO(pol.state_dict(), val.state_dict())
    opt = torch.optim.Adam(list(pol.parameters()) + list(val.parameters()), lr=1e-4)
    params = list(pol.parameters()) + list(val.parameters())
    mb_rows = B // 60
    perm = torch.randperm(B, device=dev)

    def torch_mb(mb):
        loss, _ = ex.ppo_loss(pol, val, obs[mb], act[mb], logp[mb], vals[mb], ret[mb], adv[mb])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 0.5)
        opt.step()

    def fused_mb(mb):
        fused.minibatch(obs, act, logp, vals, ret, adv, mb)
        fused.apply()

    def torch_gae():
        with torch.no_grad():
            a = torch.zeros_like(rew); gae = torch.zeros(n, device=dev)
            vb = vals.view(T, n)
            for t in reversed(range(T)):
                nv = last_v if t == T - 1 else vb[t + 1]
                nd = 1.0 - done[t]
                delta = rew[t] + ex.GAMMA * nv * nd - vb[t]
                gae = delta + ex.GAMMA * ex.LAM * nd * gae
                a[t] = gae
            return a + vb

    vb = vals.view(T, n)
    res = {"envs": n, "rollouts": T, "minibatch_rows": mb_rows, "device": torch.cuda.get_device_name(0)}
    if args.gate:
        perms = [torch.randperm(B, device=dev) for _ in range(4)]
        items = {"ungated_a": {}, "gated_no_stop": dict(kl_early_stop=1e30), "ungated_b": {},
                 "gated_stop_at_first": dict(kl_early_stop=1e-30)}
        order = list(items)
        times = {k: [] for k in items}
        info = {}
        for r in range(-2, args.gate_reps):             # two warm-up rounds
            for k in (order if r % 2 == 0 else order[::-1]):
                t = timed(lambda: fused.update(obs, act, logp, vals, ret, adv, perms=perms, **items[k]))
                if r >= 0:
                    times[k].append(t)
                info[k] = fused.last_update
        for k in items:
            res["update_" + k] = dict(summary(times[k]), last_update=info[k])
        a, b = res["update_ungated_a"]["median_ms"], res["update_ungated_b"]["median_ms"]
        res["ungated_spread_ms"] = abs(a - b)
        res["gated_no_stop_minus_ungated_ms"] = res["update_gated_no_stop"]["median_ms"] - 0.5 * (a + b)
        res["skipped_minibatch_and_apply_us"] = 1e3 * res["update_gated_stop_at_first"]["median_ms"] / (4 * 60)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    mbs = [perm[i * mb_rows:(i + 1) * mb_rows].contiguous() for i in range(60)]
    for i in range(3):                                  # warm-up
        fused_mb(mbs[i])
        if not args.fused_only:
            torch_mb(mbs[i])
    tf, tt = [], []
    for r in range(args.reps):
        tf.append(timed(lambda: fused_mb(mbs[r % 60])))
        if not args.fused_only:
            tt.append(timed(lambda: torch_mb(mbs[r % 60])))
    res["minibatch_fused"] = summary(tf)
    if tt:
        res["minibatch_torch"] = summary(tt)
    uf, ut = [], []
    for r in range(args.update_reps):
        uf.append(timed(lambda: fused.update(obs, act, logp, vals, ret, adv)))
        if not args.fused_only:
            def torch_update():
                for _ in range(4):
                    for mb in torch.randperm(B, device=dev).chunk(60):
                        torch_mb(mb)
            ut.append(timed(torch_update))
    res["update_fused"] = summary(uf)
    if ut:
        res["update_torch"] = summary(ut)
    gf, gt = [], []
    for r in range(args.reps):
        gf.append(timed(lambda: fused.gae(rew, done, vb, last_v)))
        if not args.fused_only:
            gt.append(timed(torch_gae))
    res["gae_fused"] = summary(gf)
    if gt:
        res["gae_torch"] = summary(gt)
    # work from shapes, one minibatch, both networks: forward 2 m sum(N K) per network, backward dA and dW twice that again
    # (no input gradient for layer 1); reads: the gathered rows twice, the stored activations and dZs once each
    m = mb_rows
    nk = sum(a * b for a, b in SHAPES) + 128 * 2 + sum(a * b for a, b in SHAPES) + 128 * 1
    flops = 2 * m * nk + 2 * m * (nk - 80 * 961 * 2) + 2 * m * nk
    act_bytes = 4 * m * 2 * 1374
    bytes_ = 2 * 4 * m * 965 + 2 * act_bytes
    t = res["minibatch_fused"]["median_ms"] * 1e-3
    res["minibatch_model"] = {"gflop": flops / 1e9, "mbytes": bytes_ / 1e6, "tflops_at_median": flops / t / 1e12,
                              "tbytes_per_s_at_median": bytes_ / t / 1e12,
                              "note": "arithmetic intensity ~%.0f flop/byte: compute-bound on paper; the forward / backward row "
                                      "kernel runs scalar fp32 FMAs, the weight gradients run on the f32 MFMA" % (flops / bytes_)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
