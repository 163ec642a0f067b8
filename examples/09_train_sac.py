#!/usr/bin/env python3
"""Minimal SAC on the HIP-backed AAURoverEnv-v0: the reference's learning/train/sac.py with rover_sac.yaml (batch 4096, actor
and critic lr 1e-4, entropy lr 5e-3, learned entropy coefficient from 0.2, one gradient step per env step, polyak 0.005) on the
Gaussian actor of examples/04_train_ppo.py (``Net(2, True)``, imported) and two Q(s, a) critics
(``isaac_rover_orbit_amd.td3.Critic``).  Transitions live in ``td3.ReplayMemory``, one observation ring.  The update is the torch
spec ``TorchSAC`` (``--update torch``, the default) or the fused HIP update ``FusedSAC`` (``--update fused``).

Every env step: the actor's mean (``FusedSAC.actor`` on the fused kernels, or the torch actor), the action
clamp(mean + exp(clamp(log_std)) * randn), env.step, memory.add, then one gradient step on a batch drawn from the memory with
standard normal draws from ONE ``td3_explore.smooth_draw`` launch of width 4 (columns 0:2 for s', 2:4 for s), counter = the
update's number.  ``--random_timesteps`` acts uniformly at random first, ``--learning_starts`` collects without updating before
that timestep (skrl's switches of those names).

``--rollout fused`` (with ``--update fused``) replaces everything around ``env.step`` by ``sac_collect.SACCollector``: two HIP
launches per env step that act from the trainer's current actor and log_std, write the transition straight into the memory and
return the batch's indices and the update's draws; every draw is counter-based (Philox keyed by ``--seed``).

``--preprocess running`` is rover_sac.yaml's ``state_preprocessor: RunningStandardScaler``: the policy acts on standardised rows,
the memory keeps the raw ones, and every update standardises (and trains the statistics on) its sampled ``s`` and ``s'``
(``offpolicy_scaled.FusedScaledSAC`` / ``TorchScaledSAC``; the collector takes the trainer's scaler).  ``--save`` then writes skrl's
``state_preprocessor`` entry beside the networks and ``--resume`` reads it back.

    python examples/09_train_sac.py --num_envs 4096 --timesteps 2000 --update fused --out sac.jsonl
    python examples/09_train_sac.py --num_envs 4096 --timesteps 2000 --update fused --rollout fused
    python examples/09_train_sac.py --preprocess running --update fused --rollout fused --save sac.pt
    python examples/09_train_sac.py --preprocess running --update fused --rollout fused --resume sac.pt
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isaac_rover_orbit_amd.sac import HPARAMS, LOG_STD_MAX, LOG_STD_MIN, FusedSAC, TorchSAC  # noqa: E402
from isaac_rover_orbit_amd.offpolicy_scaled import FusedScaledSAC, TorchScaledSAC  # noqa: E402
from isaac_rover_orbit_amd.td3 import Critic, ReplayMemory  # noqa: E402
from isaac_rover_orbit_amd import tracker as tracking  # noqa: E402
from isaac_rover_orbit_amd.envs.rover_env import LOG_KEYS  # noqa: E402

_spec = importlib.util.spec_from_file_location("train_ppo_example", os.path.join(ROOT, "examples", "04_train_ppo.py"))
ppo_example = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ppo_example)

LOGGED = ("critic_loss", "q1_mean", "q2_mean", "y_mean", "policy_loss", "entropy_loss", "logp_mean", "alpha")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--batch_size", type=int, default=HPARAMS["batch_size"])
    ap.add_argument("--memory_size", type=int, default=None, help="memory slots (default 2 x batch_size, as the reference)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--log_every", type=int, default=50, help="env steps per logged line (the fused path syncs only then)")
    ap.add_argument("--out", default=None, help="write the logged statistics as JSON lines")
    ap.add_argument("--save", default=None, help="write a checkpoint (policy, critic_1, ..., log_entropy_coefficient)")
    ap.add_argument("--update", choices=("torch", "fused"), default="torch",
                    help="SAC update: the torch spec (TorchSAC) or the fused HIP kernels (FusedSAC)")
    ap.add_argument("--rollout", choices=("torch", "fused"), default="torch",
                    help="collection around env.step: torch ops, or the fused collector (SACCollector; needs --update fused)")
    ap.add_argument("--random_timesteps", type=int, default=HPARAMS["random_timesteps"],
                    help="env steps of uniform random actions before the actor acts (skrl random_timesteps)")
    ap.add_argument("--learning_starts", type=int, default=HPARAMS["learning_starts"],
                    help="collect without an update before this timestep (skrl learning_starts)")
    ap.add_argument("--preprocess", choices=("none", "running"), default="none",
                    help="state_preprocessor of rover_sac.yaml: none, or skrl's RunningStandardScaler on the 965-wide states")
    ap.add_argument("--resume", default=None, help="start from a checkpoint written by --save (with --preprocess running: its "
                                                   "state_preprocessor entry too)")
    tracking.add_arguments(ap)
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.rollout == "fused" and args.update != "fused":
        ap.error("--rollout fused needs --update fused (the collector reads the fused trainer's actor and log_std)")
    from isaac_rover_orbit_amd import terrain as T
    from isaac_rover_orbit_amd.cfg import RoverEnvCfg
    from isaac_rover_orbit_amd.envs import RoverEnv
    from isaac_rover_orbit_amd.td3_explore import smooth_draw
    torch.manual_seed(args.seed)
    dev = torch.device("cuda")
    n, M = args.num_envs, args.memory_size or 2 * args.batch_size
    print(json.dumps({"memory_slots": M, "num_envs": n, "memory_gb": ReplayMemory.nbytes(M, n) / 1e9}), flush=True)
    terrain = T.make_procedural_terrain((2048, 2048), seed=1234)
    terrain.make_spawns(2 * n)
    cfg = RoverEnvCfg(); cfg.scene.num_envs = n; cfg.terrain.kind = "custom"
    env = RoverEnv(cfg, terrain=terrain)
    policy, critic_1, critic_2 = ppo_example.Net(2, True).to(dev), Critic().to(dev), Critic().to(dev)
    memory = ReplayMemory(M, n, device=dev)
    fused = spec = scaled = None
    ck = torch.load(args.resume, map_location="cpu", weights_only=False) if args.resume else None
    if args.update == "fused":
        fused = FusedSAC.from_checkpoint(ck) if ck else FusedSAC(policy.state_dict(), critic_1.state_dict(), critic_2.state_dict())
    else:
        spec = TorchSAC.from_checkpoint(ck, policy, critic_1, critic_2) if ck else TorchSAC(policy, critic_1, critic_2)
    if args.preprocess == "running":        # the trainer behind skrl's state scaler; ``upd`` is what updates, reports and saves
        scaled = FusedScaledSAC(fused) if fused is not None else TorchScaledSAC(spec)
        if ck:
            scaled.load_state_preprocessor(ck)
    upd = scaled if scaled is not None else (fused if fused is not None else spec)
    pre = (lambda x: x) if scaled is None else (scaled.state_scaler.forward if fused is not None else scaled.state_preprocessor)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    eps = torch.empty(args.batch_size, 4, device=dev)
    EPISODE_INFO_TAGS = tracking.episode_info_tags(LOG_KEYS)      # infos["episode"], as the reference's trainer tags it
    tracker = tracking.from_args(args, n, EPISODE_INFO_TAGS, dev)     # --track: skrl's curves, kept on the device
    obs, _ = env.reset()
    col = None
    if args.rollout == "fused":
        from isaac_rover_orbit_amd.sac_collect import SACCollector
        col = SACCollector(fused.actor, fused.log_std, memory, seed=args.seed, random_timesteps=args.random_timesteps,
                           state_scaler=None if scaled is None else scaled.state_scaler)
        col.begin(obs)
    else:
        o = torch.nan_to_num(obs["policy"], neginf=0.0)
    out = open(args.out, "w") if args.out else None
    t_log, steps_log, last, updates = time.perf_counter(), 0, {}, 0
    ep_count = torch.zeros((), device=dev); ep_stats = torch.zeros(4, device=dev)
    for step in range(args.timesteps):
        if col is not None:
            obs, rew, term, trunc, info = env.step(col.act(step))
            batch = col.record(obs, rew, term, args.batch_size if step >= args.learning_starts else None)
            if batch is not None:
                upd.update(memory, *batch)
                updates += 1
        else:
            with torch.no_grad():
                if step < args.random_timesteps:
                    a = torch.rand(n, 2, device=dev, generator=gen) * 2.0 - 1.0
                else:
                    mu = fused.actor(pre(o)) if fused is not None else policy(pre(o))
                    log_std = fused.log_std if fused is not None else policy.log_std_parameter
                    sigma = log_std.clamp(LOG_STD_MIN, LOG_STD_MAX).exp()
                    a = (mu + sigma * torch.randn(n, 2, device=dev, generator=gen)).clamp(-1.0, 1.0)
            obs, rew, term, trunc, info = env.step(a)
            o_next = torch.nan_to_num(obs["policy"], neginf=0.0)
            memory.add(o, a, rew, o_next, term)
            o = o_next
        lv = env.episode_log_vector
        ep_count += lv[13]; ep_stats += torch.where(lv[13] > 0, lv[7:11], torch.zeros_like(lv[7:11]))
        if tracker is not None:             # skrl's curves on the device: the raw reward, lv behind the env's own log reduction
            tracker.step(rew, term, trunc)
            tracker.track_vector(EPISODE_INFO_TAGS, lv)
            tracker.post_interaction(step)
        if col is None and step >= args.learning_starts:
            idx = memory.sample_indices(args.batch_size, gen)
            smooth_draw(args.seed, updates, 1.0, eps)
            if fused is not None:
                upd.update(memory, idx, eps)
            else:
                last = upd.update(memory, idx, eps)
            updates += 1
        steps_log += 1
        if (step + 1) % args.log_every == 0 or step + 1 == args.timesteps:
            if fused is not None and updates:
                s = upd.stats()
                last = {k: s[k] for k in LOGGED + ("critic_step", "actor_step", "entropy_step", "bad_index")}
            torch.cuda.synchronize()
            dt = time.perf_counter() - t_log
            st = {"timestep": step + 1, "memory_rows": len(memory), "updates": updates, **last,
                  "episodes": ep_count.item(), "time_out": ep_stats[0].item(), "success": ep_stats[1].item(),
                  "far": ep_stats[2].item(), "collision": ep_stats[3].item(), "env_steps_per_s": steps_log * n / dt}
            print(json.dumps(st), flush=True)
            if out:
                out.write(json.dumps(st) + "\n"); out.flush()
            t_log, steps_log = time.perf_counter(), 0
    if out:
        out.close()
    if args.save:
        torch.save(upd.state_dict() if fused is not None else upd.checkpoint(), args.save)
    env.close()
    return last


if __name__ == "__main__":
    main()
