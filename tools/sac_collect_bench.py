#!/usr/bin/env python3
"""Dev tool (GPU box): the trainer-visible SAC loop at 4096 envs on the config-2 terrain, after a pre-roll.

Two loops, alternated in one process (the same env and the same FusedSAC, so both see the same device state):
  torch  -- the glue of examples/09_train_sac.py --rollout torch: actor launch, clamp / exp / randn / multiply / add / clamp,
            nan_to_num, ReplayMemory.add (ring copy, three small copies, the host scalar into ring_pos), randint, one smooth_draw
  fused  -- isaac_rover_orbit_amd.sac_collect.SACCollector: collector.act, env.step, collector.record
each without the update and with FusedSAC.update behind every step.  Per-step wall time over a window that ends in a device
synchronise; the median and the spread over the rounds are reported, and whether the collector loop's median lies below the torch
loop's by more than the two spreads together.  A second section times the act kernel beside rover_policy_forward on the same rows,
back to back; a third counts the kernel launches of one step of each loop with torch's profiler.

    python tools/sac_collect_bench.py [--rounds 6] [--preroll 500] [--out profiles/sac_collect_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isaac_rover_orbit_amd import terrain as T  # noqa: E402
from isaac_rover_orbit_amd.cfg import RoverEnvCfg  # noqa: E402
from isaac_rover_orbit_amd.envs import RoverEnv  # noqa: E402
from isaac_rover_orbit_amd.sac import LOG_STD_MAX, LOG_STD_MIN, FusedSAC  # noqa: E402
from isaac_rover_orbit_amd.sac_collect import MEAN, SACCollector, collect_act, collect_record, default_hparams  # noqa: E402
from isaac_rover_orbit_amd.td3 import Critic, ReplayMemory  # noqa: E402
from isaac_rover_orbit_amd.td3_explore import smooth_draw  # noqa: E402


def load_example():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_ppo_example", os.path.join(ROOT, "examples", "04_train_ppo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernel_times(actor, log_std, rows, reps=300):
    """us per launch, back to back on one stream: rover_policy_forward, the act kernel in MEAN and in SAMPLE mode, and the record
    kernel on the same rows with a batch of n indices and draws."""
    n = rows.shape[0]
    f = dict(dtype=torch.float32, device="cuda")
    mean, act, env_act = (torch.empty(n, 2, **f) for _ in range(3))
    sample, plain = default_hparams(), default_hparams()
    plain.mode = MEAN
    slot, rew, rew_out, eps = torch.empty_like(rows), torch.zeros(n, **f), torch.empty(n, **f), torch.empty(n, 4, **f)
    term, term_out = torch.zeros(n, dtype=torch.bool, device="cuda"), torch.empty(n, dtype=torch.bool, device="cuda")
    pos, idx = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
    forms = {"policy_forward": lambda: actor(rows, mean),
             "act_mean": lambda: collect_act(actor, log_std, rows, 1, plain, act, env_act),
             "act_sample": lambda: collect_act(actor, log_std, rows, 1, sample, act, env_act),
             "record": lambda: collect_record(rows, slot, sample, 1, rew=rew, terminated=term, rew_out=rew_out, term_out=term_out,
                                              ring_pos_entry=pos, ring_pos_value=3, idx_out=idx, mem_rows=17 * n, eps_out=eps)}
    res = {name: [] for name in forms}
    for _ in range(5):                               # alternate the forms; each window ends in a synchronise
        for name, fn in forms.items():
            for _ in range(30):
                fn()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / reps * 1e6)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in res.items()}


def count_launches(fn, steps=10):
    """Kernel launches per call of ``fn`` over ``steps`` calls, from torch's profiler (device-side kernel events)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower()]
    copies = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" in e.name.lower()]
    return len(kernels) / steps, len(copies) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--memory_size", type=int, default=16, help="memory slots: small enough to fit (17 ring slots of 15.8 MB at 4096 envs)")
    ap.add_argument("--batch_size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--preroll", type=int, default=500)
    ap.add_argument("--steps", type=int, default=600, help="env steps per window without the update")
    ap.add_argument("--update_steps", type=int, default=150, help="env steps per window with the update")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sac_collect_bench needs a ROCm GPU: nothing is measured without one")
    if args.rounds < 5:
        sys.exit("at least five windows per loop")
    n, B = args.num_envs, args.batch_size
    dev = torch.device("cuda")
    ex = load_example()
    torch.manual_seed(42)
    fused = FusedSAC(ex.Net(2, True).state_dict(), Critic().state_dict(), Critic().state_dict())
    actor = fused.actor
    ter = T.make_procedural_terrain((2048, 2048), seed=1234, sigma_z=0.15, n_rocks=400)      # bench.py config 2
    ter.make_spawns(2 * n, seed=41)
    cfg = RoverEnvCfg(); cfg.scene.num_envs = n; cfg.terrain.kind = "custom"
    env = RoverEnv(cfg, terrain=ter)
    obs, _ = env.reset()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device=dev).manual_seed(1)
    for _ in range(args.preroll):
        obs, *_ = env.step(torch.rand(n, 2, device=dev, generator=g) * 2 - 1)
    torch.cuda.synchronize()
    rows = torch.nan_to_num(obs["policy"], neginf=0.0)
    kt = kernel_times(actor, fused.log_std, rows)
    say(f"[kernels, back to back, n={n}] us per launch, median (min .. max) of 5 windows x 300")
    for name, (med, lo, hi) in kt.items():
        say(f"  {name:16s} {med:7.2f}  ({lo:.2f} .. {hi:.2f})")

    mem_t, mem_f = ReplayMemory(args.memory_size, n, device=dev), ReplayMemory(args.memory_size, n, device=dev)
    collector = SACCollector(actor, fused.log_std, mem_f, seed=42)
    gen = torch.Generator(device=dev).manual_seed(42)
    eps = torch.empty(B, 4, device=dev)
    state = {"obs": obs, "o": rows, "updates": 0, "t": 0}

    def torch_step(update):                           # examples/09_train_sac.py, the loop of --rollout torch
        o = state["o"]
        with torch.no_grad():
            mu = actor(o)
            sigma = fused.log_std.clamp(LOG_STD_MIN, LOG_STD_MAX).exp()
            a = (mu + sigma * torch.randn(n, 2, device=dev, generator=gen)).clamp(-1.0, 1.0)
        obs, rew, term, trunc, info = env.step(a)
        o_next = torch.nan_to_num(obs["policy"], neginf=0.0)
        mem_t.add(o, a, rew, o_next, term)
        state["o"], state["obs"] = o_next, obs
        idx = mem_t.sample_indices(B, gen)
        smooth_draw(42, state["updates"], 1.0, eps)
        state["updates"] += 1
        if update:
            fused.update(mem_t, idx, eps)

    def fused_step(update):                           # ... of --rollout fused
        obs, rew, term, trunc, info = env.step(collector.act(state["t"]))
        idx, e = collector.record(obs, rew, term, B)
        state["obs"] = obs
        state["t"] += 1
        if update:
            fused.update(mem_f, idx, e)

    def enter(name):                                  # the loop that takes over starts from the env's current rows
        if name.startswith("fused"):
            collector.begin(state["obs"])
        else:
            state["o"] = torch.nan_to_num(state["obs"]["policy"], neginf=0.0)

    loops = {"torch": (torch_step, False), "fused": (fused_step, False), "torch + update": (torch_step, True),
             "fused + update": (fused_step, True)}
    per_step = {k: [] for k in loops}
    for k, (fn, upd) in loops.items():                # warm every shape; fill both memories past the wrap
        enter(k)
        for _ in range(args.memory_size + 4):
            fn(upd)
    for r in range(args.rounds):
        for k, (fn, upd) in loops.items():
            steps = args.update_steps if upd else args.steps
            enter(k)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(steps):
                fn(upd)
            torch.cuda.synchronize()
            per_step[k].append((time.perf_counter() - t0) / steps * 1e6)
    say(f"[SAC loop, n={n}, batch {B}, memory_size {args.memory_size}, pre-roll {args.preroll} steps, {args.rounds} alternated windows "
        f"of {args.steps} steps ({args.update_steps} with the update)] us per env step (host clock around a window that ends in a "
        "device synchronise)")
    for k, v in per_step.items():
        say(f"  {k:15s} median {statistics.median(v):8.2f}  min {min(v):8.2f}  max {max(v):8.2f}  spread {max(v) - min(v):7.2f}   "
            f"all: {' '.join(f'{x:.1f}' for x in v)}")
    mt, mf = statistics.median(per_step["torch"]), statistics.median(per_step["fused"])
    spreads = (max(per_step["torch"]) - min(per_step["torch"])) + (max(per_step["fused"]) - min(per_step["fused"]))
    say(f"  without the update: torch - fused = {mt - mf:.2f} us per step, the two spreads together {spreads:.2f} us: "
        f"{'ACCEPTED (the gain exceeds the spreads)' if mt - mf > spreads else 'NOT ACCEPTED (the gain does not exceed the spreads)'}")
    mtu, mfu = statistics.median(per_step["torch + update"]), statistics.median(per_step["fused + update"])
    say(f"  with the update: torch - fused = {mtu - mfu:.2f} us per step of {mtu:.2f} ({100.0 * (mtu - mfu) / mtu:.1f} %); the update's "
        f"share of the loop: torch {100.0 * (mtu - mt) / mtu:.1f} %, fused {100.0 * (mfu - mf) / mfu:.1f} %")
    try:
        enter("torch")
        kt_, ct_ = count_launches(lambda: torch_step(False))
        enter("fused")
        kf_, cf_ = count_launches(lambda: fused_step(False))
        say(f"[launches per env step without the update, torch profiler, env.step's own included] torch: {kt_:.1f} kernels + {ct_:.1f} "
            f"copies; fused: {kf_:.1f} kernels + {cf_:.1f} copies")
    except Exception as e:                            # the profiler is optional equipment: say so, do not guess
        say(f"[launches per env step] not measured: {type(e).__name__}: {e}")
    env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
