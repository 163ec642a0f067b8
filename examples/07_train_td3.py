#!/usr/bin/env python3
"""Minimal TD3 on the HIP-backed AAURoverEnv-v0: the reference's learning/train/td3.py with rover_td3.yaml (batch 4096, actor
and critic lr 1e-4, RandomMemory of 2 x batch slots, one gradient step per env step, policy delay 2, polyak 0.005) on the actor
of examples/04_train_ppo.py (``Net(2, False)``, imported) and two Q(s, a) critics (``isaac_rover_orbit_amd.td3.Critic``).
Transitions live in ``td3.ReplayMemory``, one observation ring.  The update is the torch spec ``TorchTD3``
(``--update torch``, the default) or the fused HIP update ``FusedTD3`` (``--update fused``).

Every env step: the actor forward (``FusedTD3.actor`` on the fused kernels, or the torch actor), optional exploration noise,
env.step with those actions, memory.add of the same actions, then one gradient step on a batch drawn from the memory.
``--rollout fused`` (with ``--update fused``) hands all of that but env.step and the update to ``td3_explore.TD3Explorer``: two
HIP launches per env step, counter-based noise and batch indices.  That path also carries skrl's other TD3 switches: ``--noise ou``
(Ornstein-Uhlenbeck exploration noise), ``--random_timesteps`` (uniform random actions first) and ``--smooth_noise_std`` (the target
action's smoothing noise, drawn on the device).  ``--learning_starts`` collects without updating before that timestep, on either
path.  At their defaults the run is what it was without them.

``--preprocess running`` is rover_td3.yaml's ``state_preprocessor: RunningStandardScaler``: the policy acts on standardised rows,
the memory keeps the raw ones, and every update standardises (and trains the statistics on) its sampled ``s`` and ``s'``
(``offpolicy_scaled.FusedScaledTD3`` / ``TorchScaledTD3``; the collector takes the trainer's scaler).  ``--save`` then writes skrl's
``state_preprocessor`` entry beside the networks and ``--resume`` reads it back.

    python examples/07_train_td3.py --num_envs 4096 --timesteps 2000 --update fused --out td3.jsonl
    python examples/07_train_td3.py --num_envs 4096 --timesteps 2000 --update fused --rollout fused --out td3.jsonl
    python examples/07_train_td3.py --preprocess running --update fused --rollout fused --save td3.pt
    python examples/07_train_td3.py --preprocess running --update fused --rollout fused --resume td3.pt
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
from isaac_rover_orbit_amd import terrain as T  # noqa: E402
from isaac_rover_orbit_amd.cfg import RoverEnvCfg  # noqa: E402
from isaac_rover_orbit_amd.envs import RoverEnv  # noqa: E402
from isaac_rover_orbit_amd.td3 import (HPARAMS, Critic, FusedTD3, ReplayMemory, TorchTD3, exploration_scale,  # noqa: E402
                                       explore)
from isaac_rover_orbit_amd.td3_explore import TD3Explorer  # noqa: E402
from isaac_rover_orbit_amd.offpolicy_scaled import FusedScaledTD3, TorchScaledTD3  # noqa: E402
from isaac_rover_orbit_amd import tracker as tracking  # noqa: E402
from isaac_rover_orbit_amd.envs.rover_env import LOG_KEYS  # noqa: E402

_spec = importlib.util.spec_from_file_location("train_ppo_example", os.path.join(ROOT, "examples", "04_train_ppo.py"))
ppo_example = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ppo_example)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--batch_size", type=int, default=HPARAMS["batch_size"])
    ap.add_argument("--memory_size", type=int, default=None, help="memory slots (default 2 x batch_size, as the reference)")
    ap.add_argument("--exploration_noise", type=float, default=0.0,
                    help="std of Gaussian exploration noise with skrl's linear scale schedule (default 0: none, as rover_td3.yaml)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--log_every", type=int, default=50, help="env steps per logged line (the fused path syncs only then)")
    ap.add_argument("--out", default=None, help="write the logged statistics as JSON lines")
    ap.add_argument("--save", default=None, help="write a skrl-style TD3 checkpoint (policy, target_policy, critic_1, ...)")
    ap.add_argument("--update", choices=("torch", "fused"), default="torch",
                    help="TD3 update: the torch spec (TorchTD3) or the fused HIP kernels (FusedTD3)")
    ap.add_argument("--rollout", choices=("torch", "fused"), default="torch",
                    help="the glue around env.step: torch ops and ReplayMemory.add, or the fused collector (needs --update fused)")
    ap.add_argument("--noise", choices=("none", "gaussian", "ou"), default="none",
                    help="exploration noise class: skrl's GaussianNoise (std --exploration_noise) or OrnsteinUhlenbeckNoise (skrl's "
                         "defaults); none with --exploration_noise > 0 is gaussian, as before.  ou needs --rollout fused")
    ap.add_argument("--random_timesteps", type=int, default=HPARAMS["random_timesteps"],
                    help="env steps of uniform random actions before the actor acts (skrl random_timesteps; needs --rollout fused)")
    ap.add_argument("--learning_starts", type=int, default=HPARAMS["learning_starts"],
                    help="collect without an update before this timestep (skrl learning_starts)")
    ap.add_argument("--smooth_noise_std", type=float, default=0.0,
                    help="std of the target action's smoothing noise (skrl smooth_regularization_noise; 0: none; needs --rollout fused)")
    ap.add_argument("--preprocess", choices=("none", "running"), default="none",
                    help="state_preprocessor of rover_td3.yaml: none, or skrl's RunningStandardScaler on the 965-wide states")
    ap.add_argument("--resume", default=None, help="start from a checkpoint written by --save (with --preprocess running: its "
                                                   "state_preprocessor entry too)")
    tracking.add_arguments(ap)
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.rollout == "fused" and args.update != "fused":
        ap.error("--rollout fused needs --update fused (the collector runs FusedTD3's actor)")
    if args.rollout != "fused" and (args.noise == "ou" or args.random_timesteps > 0 or args.smooth_noise_std > 0):
        ap.error("--noise ou, --random_timesteps and --smooth_noise_std need --rollout fused (their draws are the collector's)")
    noise = args.noise if args.noise != "none" or args.exploration_noise <= 0 else "gaussian"
    torch.manual_seed(args.seed)
    dev = torch.device("cuda")
    n, M = args.num_envs, args.memory_size or 2 * args.batch_size
    print(json.dumps({"memory_slots": M, "num_envs": n, "memory_gb": ReplayMemory.nbytes(M, n) / 1e9,
                      "two_buffer_memory_gb": ReplayMemory.two_buffer_nbytes(M, n) / 1e9}), flush=True)
    terrain = T.make_procedural_terrain((2048, 2048), seed=1234)
    terrain.make_spawns(2 * n)
    cfg = RoverEnvCfg(); cfg.scene.num_envs = n; cfg.terrain.kind = "custom"
    env = RoverEnv(cfg, terrain=terrain)
    policy, critic_1, critic_2 = ppo_example.Net(2, False).to(dev), Critic().to(dev), Critic().to(dev)
    memory = ReplayMemory(M, n, device=dev)
    fused = spec = scaled = None
    ck = torch.load(args.resume, map_location="cpu", weights_only=False) if args.resume else None
    if args.update == "fused":
        fused = FusedTD3.from_checkpoint(ck) if ck else FusedTD3(policy.state_dict(), critic_1.state_dict(), critic_2.state_dict())
    else:
        if ck:
            for m, k in ((policy, "policy"), (critic_1, "critic_1"), (critic_2, "critic_2")):
                m.load_state_dict(ck[k])
        spec = TorchTD3(policy, critic_1, critic_2)
        for k in ("target_policy", "target_critic_1", "target_critic_2"):
            if ck and ck.get(k) is not None:
                getattr(spec, k).load_state_dict(ck[k])
    if args.preprocess == "running":        # the trainer behind skrl's state scaler; ``upd`` is what updates, reports and saves
        scaled = FusedScaledTD3(fused) if fused is not None else TorchScaledTD3(spec)
        if ck:
            scaled.load_state_preprocessor(ck)
    upd = scaled if scaled is not None else (fused if fused is not None else spec)
    pre = (lambda x: x) if scaled is None else (scaled.state_scaler.forward if fused is not None else scaled.state_preprocessor)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    EPISODE_INFO_TAGS = tracking.episode_info_tags(LOG_KEYS)      # infos["episode"], as the reference's trainer tags it
    tracker = tracking.from_args(args, n, EPISODE_INFO_TAGS, dev)     # --track: skrl's curves, kept on the device
    obs, _ = env.reset()
    collector = None
    if args.rollout == "fused":
        collector = TD3Explorer(fused.actor, memory, seed=args.seed, env_id_offset=cfg.env_id_offset, noise=noise,
                                noise_std=args.exploration_noise, random_timesteps=args.random_timesteps,
                                state_scaler=None if scaled is None else scaled.state_scaler)
        collector.begin(obs)
    else:
        o = torch.nan_to_num(obs["policy"], neginf=0.0)
    out = open(args.out, "w") if args.out else None
    t_log, steps_log, last = time.perf_counter(), 0, {}
    ep_count = torch.zeros((), device=dev); ep_stats = torch.zeros(4, device=dev)
    for step in range(args.timesteps):
        scale = None
        if args.exploration_noise > 0:
            scale = exploration_scale(step, args.timesteps, HPARAMS["exploration_initial_scale"], HPARAMS["exploration_final_scale"])
        learning = step >= args.learning_starts
        if collector is not None:
            obs, rew, term, trunc, info = env.step(collector.act(step, args.timesteps))
            idx = collector.record(obs, rew, term, args.batch_size if learning else None)   # indices over the rows filled so far
        else:
            with torch.no_grad():
                a = fused.actor(pre(o)) if fused is not None else spec.act(pre(o))
            if args.exploration_noise > 0:
                a = explore(a, args.exploration_noise * torch.randn(a.shape, device=dev, generator=gen), scale)
            obs, rew, term, trunc, info = env.step(a)
            o_next = torch.nan_to_num(obs["policy"], neginf=0.0)
            memory.add(o, a, rew, o_next, term)
            o = o_next
            idx = memory.sample_indices(args.batch_size, gen) if learning else None
        lv = env.episode_log_vector
        ep_count += lv[13]; ep_stats += torch.where(lv[13] > 0, lv[7:11], torch.zeros_like(lv[7:11]))
        if tracker is not None:             # skrl's curves on the device: the raw reward, lv behind the env's own log reduction
            tracker.step(rew, term, trunc)
            tracker.track_vector(EPISODE_INFO_TAGS, lv)
            tracker.post_interaction(step)
        if learning and fused is not None:
            smooth = collector.smooth_noise(args.batch_size, args.smooth_noise_std) if args.smooth_noise_std > 0 else None
            upd.update(memory, idx, smooth)
        elif learning:
            last = upd.update(memory, idx)
        steps_log += 1
        if (step + 1) % args.log_every == 0 or step + 1 == args.timesteps:
            if fused is not None:
                s = upd.stats()
                last = {k: s[k] for k in ("critic_loss", "q1_mean", "q2_mean", "y_mean", "policy_loss", "critic_step", "actor_step")}
            torch.cuda.synchronize()
            dt = time.perf_counter() - t_log
            st = {"timestep": step + 1, "memory_rows": len(memory), **{k: v for k, v in last.items() if k != "actor_stepped"},
                  "episodes": ep_count.item(), "time_out": ep_stats[0].item(), "success": ep_stats[1].item(),
                  "far": ep_stats[2].item(), "collision": ep_stats[3].item(), "env_steps_per_s": steps_log * n / dt}
            print(json.dumps(st), flush=True)
            if out:
                out.write(json.dumps(st) + "\n"); out.flush()
            t_log, steps_log = time.perf_counter(), 0
    if args.save:
        torch.save(upd.state_dict() if fused is not None else upd.checkpoint(), args.save)
    env.close()


if __name__ == "__main__":
    main()
