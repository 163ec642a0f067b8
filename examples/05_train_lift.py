#!/usr/bin/env python3
"""PPO on the HIP-backed FrankaCubeLift-v0 with the reference's skrl setup (rover_envs/envs/manipulation/config/franka/agents/
skrl_ppo_cfg.yaml): ELU networks 36 -> 256 -> 128 -> 64 -> {8, 1}, RunningStandardScaler on states and values, rewards x 0.01,
24 rollouts, 8 epochs, 24 minibatches, lr 1e-4 with KLAdaptiveRL, KL early stop 0.008, value-loss scale 2, grad-norm clip 1.0.
Rollouts run on the fused kernels (env.step = HIP, policy mean and value = one HIP forward each); the update is either the
torch spec (``--update torch``: isaac_rover_orbit_amd.lift_ppo.TorchLiftPPO, plain autograd + torch.optim.Adam) or the fused HIP
update (``--update fused``: FusedLiftPPO; the rollout reads the trainer's parameters and scalers directly).  ``--rollout fused``
(with ``--update fused``) replaces the per-step torch glue around ``env.step`` with isaac_rover_orbit_amd.lift_rollout's
LiftRolloutCollector: one launch for scale + act + sample + log-prob, one for the reward / done record and the episode tally; its
action noise is counter-based (Philox), so the curve follows ``--rollout torch`` statistically, not bit for bit.  A stand-in for
the reference's skrl trainer, which needs packages that are not part of this repository.

    python examples/05_train_lift.py --update fused --rollout fused --num_envs 4096 --iterations 100 --out curve.jsonl
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isaac_rover_orbit_amd import lift_ppo as LP  # noqa: E402
from isaac_rover_orbit_amd import tracker as tracking  # noqa: E402
from isaac_rover_orbit_amd.envs.lift_env import LOG_KEYS, FrankaCubeLiftEnv, LiftEnvCfg, REWARD_ORDER, TERMINATION_ORDER  # noqa: E402

LOG_NAMES = [f"Episode Reward/{k}" for k in REWARD_ORDER] + [f"Episode Termination/{k}" for k in TERMINATION_ORDER]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--rollouts", type=int, default=24)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None, help="write the per-iteration statistics as JSON lines")
    ap.add_argument("--save", default=None, help="write a skrl-style checkpoint (policy, value, both preprocessors)")
    ap.add_argument("--update", choices=("torch", "fused"), default="torch",
                    help="PPO update: the torch spec (autograd + torch.optim.Adam) or the fused HIP kernels")
    ap.add_argument("--rollout", choices=("torch", "fused"), default="torch",
                    help="per-step rollout glue: torch ops, or the fused HIP collector (needs --update fused)")
    tracking.add_arguments(ap)
    args = ap.parse_args()
    if args.rollout == "fused" and args.update != "fused":
        ap.error("--rollout fused requires --update fused")
    torch.manual_seed(args.seed)
    dev = torch.device("cuda")
    n, Tn = args.num_envs, args.rollouts
    cfg = LiftEnvCfg(); cfg.scene.num_envs = n; cfg.seed = args.seed; cfg.log_reduction = "every_step"
    env = FrankaCubeLiftEnv(cfg)
    policy, value = LP.LiftMLP(LP.ACT_DIM, log_std=True), LP.LiftMLP(1)
    hp = LP.default_hparams()
    if args.update == "fused":
        fused = LP.FusedLiftPPO(policy.state_dict(), value.state_dict(), lr=1e-4)
        spec = None
    else:
        fused = None
        spec = LP.TorchLiftPPO(policy, value, lr=1e-4)

    obs_buf = torch.empty(Tn, n, LP.OBS_DIM, device=dev)
    act_buf = torch.empty(Tn, n, LP.ACT_DIM, device=dev)
    logp_buf, val_buf, rew_buf, done_buf = (torch.empty(Tn, n, device=dev) for _ in range(4))
    col = None
    if args.rollout == "fused":                 # the collector's own (T, n, ...) buffers go straight into gae / update
        from isaac_rover_orbit_amd.lift_rollout import LiftRolloutCollector
        col = LiftRolloutCollector(fused, n, Tn, seed=args.seed)
        obs_buf, act_buf, logp_buf, val_buf, rew_buf, done_buf = col.obs, col.actions, col.logp, col.val, col.rew, col.done
    obs, _ = env.reset()
    o = obs["policy"].clone()
    out = open(args.out, "w") if args.out else None
    log = env._log
    EPISODE_INFO_TAGS = tracking.episode_info_tags(LOG_KEYS)      # infos["episode"], as the reference's trainer tags it
    tracker = tracking.from_args(args, n, EPISODE_INFO_TAGS, dev)     # --track: skrl's curves, kept on the device
    for it in range(args.iterations):
        t0 = time.perf_counter()
        if fused is None:
            actor, critic = LP.lift_net(policy.state_dict()), LP.lift_net(value.state_dict())
            state_pre = lambda x: spec.state_preprocessor(x)                                   # noqa: E731
            value_inv = lambda v: spec.value_preprocessor(v, inverse=True)                     # noqa: E731
            log_std = policy.log_std_parameter.detach()
        else:                                   # the trainer's own parameters and scalers: nothing to re-pack
            actor, critic = fused.actor, fused.critic
            state_pre = lambda x: fused.standardize(x, "state")                                # noqa: E731
            value_inv = lambda v: fused.standardize(v, "value", inverse=True)                  # noqa: E731
            log_std = fused.log_std
        ls = log_std.clamp(-20.0, 2.0)
        std = ls.exp()
        ep_sum = torch.zeros(8, device=dev); ep_count = torch.zeros((), device=dev)
        if col is not None:
            col.reset_tally()
            ep_sum, ep_count = col.ep_sum, col.ep_count
        with torch.no_grad():
            for t in range(Tn if col is None else 0):
                s = state_pre(o)
                mean = actor(s)
                a = mean + std * torch.randn_like(mean)                   # clip_actions: False
                logp_buf[t] = LP.gaussian_logp(mean, log_std, a)
                val_buf[t] = value_inv(critic(s)).squeeze(1)
                obs_buf[t], act_buf[t] = o, a
                obs, rew, term, trunc, _ = env.step(a)
                o = obs["policy"]
                rew_buf[t] = rew * hp.reward_scale                        # rewards_shaper_scale
                done_buf[t] = (term | trunc).float()
                k = log[8]                                                # envs reset in this step; log[0:8] are their means
                ep_sum += torch.where(k > 0, log[0:8] * torch.where(torch.arange(8, device=dev) < 6, k, 1.0), 0.0)
                ep_count += k
                if tracker is not None:                                   # the env's raw reward; log is reduced every step
                    tracker.step(rew, term, trunc)
                    tracker.track_vector(EPISODE_INFO_TAGS, log)
                    tracker.post_interaction(it * Tn + t)
            for t in range(Tn if col is not None else 0):                 # the same steps, two launches around env.step
                obs, rew, term, trunc, _ = env.step(col.act(t, o))
                o = obs["policy"]
                col.record(t, rew, term, trunc, log)
                if tracker is not None:                                   # the env's raw reward; log is reduced every step
                    tracker.step(rew, term, trunc)
                    tracker.track_vector(EPISODE_INFO_TAGS, log)
                    tracker.post_interaction(it * Tn + t)
            torch.cuda.synchronize(); t_roll = time.perf_counter() - t0
            last_v = col.last_value(o) if col is not None else value_inv(critic(state_pre(o))).squeeze(1)
            if fused is not None:
                adv, ret = fused.gae(rew_buf, done_buf, val_buf, last_v)
            else:
                adv, ret = LP.gae_torch(rew_buf, done_buf, val_buf, last_v, hp.gamma, hp.lam)
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            if fused is not None:
                val_s = fused.standardize(val_buf.reshape(-1, 1).contiguous(), "value", train=True).reshape(Tn, n)
                ret_s = fused.standardize(ret.reshape(-1, 1).contiguous(), "value", train=True).reshape(Tn, n)
            else:
                val_s = spec.value_preprocessor(val_buf.reshape(-1, 1), train=True).reshape(Tn, n)
                ret_s = spec.value_preprocessor(ret.reshape(-1, 1), train=True).reshape(Tn, n)
        t1 = time.perf_counter()
        B = Tn * n
        flat = [x.reshape(B, *x.shape[2:]).contiguous() for x in (obs_buf, act_buf, logp_buf, val_s, ret_s, adv)]
        if fused is not None:
            kls, lr = fused.update(*flat)
            stopped = fused.stopped_epochs
        else:
            kls, lr = spec.update(*flat)
            stopped = spec.stopped_epochs
        torch.cuda.synchronize()
        t_upd = time.perf_counter() - t1
        cnt = ep_count.item()
        sums = ep_sum.cpu().tolist()
        st = {"iteration": it, "update": args.update, "mean_step_reward": rew_buf.mean().item() / hp.reward_scale, "episodes": cnt}
        for i, name in enumerate(LOG_NAMES):
            st[name] = sums[i] / cnt if (i < 6 and cnt > 0) else (sums[i] if i >= 6 else None)
        st.update({"kl": kls[-1], "kl_epochs": kls, "lr": lr, "stopped_epochs_total": stopped, "rollout_s": t_roll,
                   "update_s": t_upd, "iteration_s": time.perf_counter() - t0})
        print(json.dumps(st), flush=True)
        if out:
            out.write(json.dumps(st) + "\n"); out.flush()
    if args.save:
        torch.save(fused.state_dict() if fused is not None else spec.state_dict(), args.save)
    env.close()


if __name__ == "__main__":
    main()
