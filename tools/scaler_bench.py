#!/usr/bin/env python3
"""Dev tool (GPU box): what skrl's running scalers cost the rover's PPO at the reference's size (4096 envs, 60 rollouts).

Two sections, each alternating its forms in one process over windows that end in a device synchronise (host clock); the median
and the spread over the windows are reported:

  act     -- one rollout step without the env, on fixed raw rows with misses (-inf):
               plain   rollout.RolloutCollector.act                   (one launch, no scalers: the floor)
               fused   rollout_scaled.ScaledRolloutCollector.act      (three launches)
               glue    the torch glue of examples/04_train_ppo.py --preprocess running --rollout torch on the GPU: nan_to_num,
                       lift_ppo.RunningStandardScaler, RoverNet actor and critic, torch.randn, log-prob, inverse, buffer copies
               spec    rollout_scaled.TorchScaledRollout.act on the GPU (its draws are numpy Philox on the host)
  update  -- one PPO update of 60 x 4096 rows, 4 epochs x 60 minibatches:
               plain   ppo.FusedPPO.update                            (no scalers: the floor)
               fused   ppo_scaled.FusedScaledPPO.standardize_values + .update
               torch   ppo_scaled.TorchScaledPPO.standardize_values + .update on the GPU

    python tools/scaler_bench.py [--rounds 5] [--out profiles/scaler_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isaac_rover_orbit_amd.lift_ppo import RunningStandardScaler  # noqa: E402
from isaac_rover_orbit_amd.ppo import FusedPPO  # noqa: E402
from isaac_rover_orbit_amd.ppo_scaled import FusedScaledPPO, TorchScaledPPO  # noqa: E402
from isaac_rover_orbit_amd.rollout import RolloutCollector  # noqa: E402
from isaac_rover_orbit_amd.rollout_scaled import ScaledRolloutCollector, TorchScaledRollout  # noqa: E402


def load_example():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_ppo_example", os.path.join(ROOT, "examples", "04_train_ppo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def windows(forms, rounds, say, unit):
    """forms: {name: (fn, calls per window)}.  Alternates the forms; returns {name: [seconds per call]}."""
    res = {k: [] for k in forms}
    for k, (fn, _) in forms.items():            # warm every shape
        fn(); fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, (fn, calls) in forms.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            res[k].append((time.perf_counter() - t0) / calls)
    scale = {"us": 1e6, "ms": 1e3}[unit]
    for k, v in res.items():
        v = [x * scale for x in v]
        say(f"  {k:6s} median {statistics.median(v):10.2f} {unit}  min {min(v):10.2f}  max {max(v):10.2f}  spread {max(v) - min(v):8.2f}   "
            f"({forms[k][1]} calls per window)  all: {' '.join(f'{x:.2f}' for x in v)}")
    return res


def verdict(res, a, b, say, unit):
    scale = {"us": 1e6, "ms": 1e3}[unit]
    ma, mb = statistics.median(res[a]) * scale, statistics.median(res[b]) * scale
    spreads = (max(res[a]) - min(res[a]) + max(res[b]) - min(res[b])) * scale
    say(f"  {a} - {b} = {ma - mb:.2f} {unit} ({ma / mb:.2f} x); the two spreads together {spreads:.2f} {unit}: "
        f"{'the difference exceeds the spreads' if abs(ma - mb) > spreads else 'the difference does NOT exceed the spreads'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--rollouts", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--act_calls", type=int, default=2000, help="act calls per window of the fused forms")
    ap.add_argument("--skip_update", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scaler_bench needs a ROCm GPU: nothing is measured without one")
    if args.rounds < 5:
        sys.exit("at least five windows per form")
    n, Tn = args.num_envs, args.rollouts
    dev = torch.device("cuda")
    ex = load_example()
    torch.manual_seed(42)
    policy, value = ex.Net(2, True), ex.Net(1, False)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device=dev).manual_seed(1)
    col = torch.rand(965, device=dev, generator=g)
    raw = torch.randn(n, 965, device=dev, generator=g) * (0.2 + 4.0 * col) + (col - 0.5) * 6.0
    raw[:, 4:964][torch.rand(n, 960, device=dev, generator=g) < 1.0 / 16.0] = float("-inf")      # the scanner's misses

    # ---------------------------------------------------------------------------------------------------------------- act
    plain_tr = FusedPPO(policy.state_dict(), value.state_dict())
    tr = FusedScaledPPO(policy.state_dict(), value.state_dict())
    tr.state_scaler.train(torch.nan_to_num(raw, neginf=0.0))
    tr.value_scaler.train(torch.randn(n, 1, device=dev, generator=g) * 3 + 1)
    c_plain = RolloutCollector(plain_tr.actor, plain_tr.critic, plain_tr.log_std, n, Tn)
    c_fused = ScaledRolloutCollector(tr.actor, tr.critic, tr.log_std, tr.state_scaler, tr.value_scaler, n, Tn)
    ts, tv = RunningStandardScaler(965, device=dev), RunningStandardScaler(1, device=dev)
    ts.load_state_dict(tr.state_scaler.state_dict()); tv.load_state_dict(tr.value_scaler.state_dict())
    c_spec = TorchScaledRollout(tr.actor, tr.critic, tr.log_std, ts, tv, n, Tn, device=raw.device)
    glue = {k: torch.empty(Tn, n, *s, device=dev) for k, s in (("obs", (965,)), ("act", (2,)), ("logp", ()), ("val", ()))}
    step = {"t": 0}

    def glue_act():                             # examples/04_train_ppo.py, the loop of --rollout torch --preprocess running
        t = step["t"] = (step["t"] + 1) % Tn
        with torch.no_grad():
            o = torch.nan_to_num(raw, neginf=0.0)
            log_std = tr.log_std.clamp(-20.0, 2.0)
            std = log_std.exp()
            s = ts(o)
            mean = tr.actor(s)
            a = mean + std * torch.randn_like(mean)
            glue["logp"][t] = (-0.5 * ((a - mean) / std) ** 2 - log_std - 0.9189385332).sum(1)
            glue["val"][t] = tv(tr.critic(s), inverse=True).squeeze(1)
            glue["obs"][t], glue["act"][t] = o, a
            return a.clamp(-1.0, 1.0)

    def col_act(c):
        def fn():
            t = step["t"] = (step["t"] + 1) % Tn
            c.act(t, raw)
        return fn

    say(f"[act, n={n}, no env, {args.rounds} alternated windows] us per call (host clock around a window that ends in a device "
        "synchronise)")
    forms = {"plain": (col_act(c_plain), args.act_calls), "fused": (col_act(c_fused), args.act_calls),
             "glue": (glue_act, max(args.act_calls // 4, 1)), "spec": (col_act(c_spec), max(args.act_calls // 40, 1))}
    res = windows(forms, args.rounds, say, "us")
    verdict(res, "fused", "plain", say, "us")
    verdict(res, "glue", "fused", say, "us")
    verdict(res, "spec", "fused", say, "us")
    nbytes = 3 * n * 965 * 4
    say(f"  the scalers' own traffic per call: {nbytes / 1e6:.1f} MB (the raw rows read, the sanitised and the standardised rows "
        f"written), plus the standardised rows read again by the act kernel")

    # ------------------------------------------------------------------------------------------------------------- update
    if not args.skip_update:
        B = Tn * n
        obs = torch.empty(B, 965, device=dev)
        for i in range(0, B, n):                # rows like the act section's, without the misses (the buffer holds sanitised rows)
            obs[i:i + n] = torch.randn(n, 965, device=dev, generator=g) * (0.2 + 4.0 * col) + (col - 0.5) * 6.0
        act = torch.randn(B, 2, device=dev, generator=g)
        logp = torch.randn(B, device=dev, generator=g) * 0.3 - 2.0
        val = torch.randn(B, device=dev, generator=g) * 3 + 1
        ret = val + torch.randn(B, device=dev, generator=g)
        adv = torch.randn(B, device=dev, generator=g)
        tt = TorchScaledPPO(ex.Net(2, True), ex.Net(1, False), device=dev)

        def upd_plain():
            plain_tr.update(obs, act, logp, val, ret, adv)

        def upd_fused():
            v, r = tr.standardize_values(val, ret)
            tr.update(obs, act, logp, v, r, adv)

        def upd_torch():
            v, r = tt.standardize_values(val, ret)
            tt.update(obs, act, logp, v, r, adv)

        say(f"[update, {Tn} x {n} = {B} rows, 4 epochs x 60 minibatches, {args.rounds} alternated windows of one update] ms per update; "
            f"the rollout buffer and the image are {B * 965 * 4 / 1e6:.0f} MB each")
        res = windows({"plain": (upd_plain, 1), "fused": (upd_fused, 1), "torch": (upd_torch, 1)}, args.rounds, say, "ms")
        verdict(res, "fused", "plain", say, "ms")
        verdict(res, "torch", "fused", say, "ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
