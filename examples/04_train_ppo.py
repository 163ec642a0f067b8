#!/usr/bin/env python3
"""Minimal PPO on the HIP-backed AAURoverEnv-v0: the reference's actor / critic architecture (learning/skrl/models.py) and
hyper-parameters (learning/skrl/rover_ppo.yaml: rollouts 60, 4 epochs, 60 mini-batches, gamma 0.99, lambda 0.95,
lr 1e-4, clip 0.2, grad-norm 0.5, KL-adaptive learning rate, kl_threshold 0.008).  Rollouts run entirely on the fused
kernels (policy mean and value through ``RoverNet``, re-packed after every update; env.step = two HIP kernels); only
the PPO update itself uses torch autograd (``--update torch``, the default) or the fused HIP update of
``isaac_rover_orbit_amd.ppo.FusedPPO`` (``--update fused``: GAE, loss, backward, clip and Adam as HIP kernels; the rollout reads
the trainer's parameters directly, no re-packing).  A stand-in for the reference's skrl trainer (examples/02_train/train.py),
which needs packages that are not part of this repository.

``--preprocess running`` turns on what the reference's agent files call ``state_preprocessor`` / ``value_preprocessor``
(skrl's RunningStandardScaler on the 965-wide states and on the values): ``isaac_rover_orbit_amd.ppo_scaled`` for the update
(``TorchScaledPPO`` or ``FusedScaledPPO``) and ``isaac_rover_orbit_amd.rollout_scaled.ScaledRolloutCollector`` for the fused
rollout.  The default, ``none``, trains on the raw rows as before.

``--kl_early_stop 0.008 --scheduler none`` is rover_ppo.yaml as skrl 1.1 reads it (``kl_threshold`` is skrl's KL early stop and the
file has no ``learning_rate_scheduler``); rover_rpo.yaml is the same.  ``--rewards_shaper_scale`` / ``--time_limit_bootstrap`` are
the agent files' switches of those names.  The defaults keep this example's own reading: no early stop, KL-adaptive rate.

    python examples/04_train_ppo.py --num_envs 4096 --iterations 100
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isaac_rover_orbit_amd import terrain as T  # noqa: E402
from isaac_rover_orbit_amd.cfg import RoverEnvCfg  # noqa: E402
from isaac_rover_orbit_amd import tracker as tracking  # noqa: E402
from isaac_rover_orbit_amd.envs import RoverEnv  # noqa: E402
from isaac_rover_orbit_amd.envs.rover_env import LOG_KEYS  # noqa: E402
from isaac_rover_orbit_amd.policy import RoverNet  # noqa: E402

GAMMA, LAM, CLIP, VCLIP, KL_THR = 0.99, 0.95, 0.2, 0.2, 0.008
EPISODE_INFO_TAGS = tracking.episode_info_tags(LOG_KEYS)      # infos["episode"], as the reference's trainer tags it


class Net(nn.Module):
    """models.py:39-103 / 106-163: encoder 961 -> 80 -> 60 on obs[:, 3:-1], MLP (4 + 60) -> 256 -> 160 -> 128 -> out."""

    def __init__(self, out_dim, final_tanh):
        super().__init__()
        act = nn.LeakyReLU
        self.dense_encoder = nn.Module()
        self.dense_encoder.encoder_layers = nn.ModuleList([nn.Linear(961, 80), act(), nn.Linear(80, 60), act()])
        self.mlp = nn.ModuleList([nn.Linear(64, 256), act(), nn.Linear(256, 160), act(), nn.Linear(160, 128), act(),
                                  nn.Linear(128, out_dim)] + ([nn.Tanh()] if final_tanh else []))
        if final_tanh:
            self.log_std_parameter = nn.Parameter(torch.zeros(out_dim))

    def forward(self, s):
        e = s[:, 3:-1]
        for layer in self.dense_encoder.encoder_layers:
            e = layer(e)
        x = torch.cat([s[:, 0:4], e], 1)
        for layer in self.mlp:
            x = layer(x)
        return x


def ppo_loss(policy, value, o, a, old_lp, old_v, ret, adv, clip=CLIP, vclip=VCLIP):
    """The clipped PPO loss of one minibatch (skrl PPO with clip_predicted_values, value-loss scale 1, entropy scale 0) and the
    minibatch KL estimate ((r - 1) - log r).mean() (no gradient)."""
    mean = policy(o)
    ls = policy.log_std_parameter.clamp(-20.0, 2.0)
    lp = (-0.5 * ((a - mean) / ls.exp()) ** 2 - ls - 0.9189385332).sum(1)
    ratio = (lp - old_lp).exp()
    with torch.no_grad():
        kl = ((ratio - 1) - (lp - old_lp)).mean()
    pl = -torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv).mean()
    v = value(o).squeeze(1)
    v = old_v + (v - old_v).clamp(-vclip, vclip)
    vl = ((ret - v) ** 2).mean()
    return pl + vl, kl


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--rollouts", type=int, default=60)
    ap.add_argument("--out", default=None, help="write the per-iteration statistics as JSON lines")
    ap.add_argument("--save", default=None, help="write a skrl-style checkpoint {'policy': state_dict, 'value': state_dict}; with --preprocess running "
                                                  "also 'state_preprocessor' and 'value_preprocessor'")
    ap.add_argument("--update", choices=("torch", "fused"), default="torch",
                    help="PPO update: torch autograd + torch.optim.Adam, or the fused HIP kernels (isaac_rover_orbit_amd.ppo)")
    ap.add_argument("--rollout", choices=("torch", "fused"), default="torch",
                    help="rollout glue around env.step: torch ops with torch.randn noise, or isaac_rover_orbit_amd.rollout.RolloutCollector "
                         "(one HIP launch per step: sanitise, both networks, counter-based Gaussian actions, log-prob)")
    ap.add_argument("--preprocess", choices=("none", "running"), default="none",
                    help="running: skrl's RunningStandardScaler on states and values (state_preprocessor / value_preprocessor of "
                         "rover_ppo.yaml), as HIP kernels wherever --update / --rollout is fused")
    ap.add_argument("--kl_early_stop", type=float, default=0.0, metavar="F",
                    help="skrl's KL early stop (its kl_threshold): an epoch stops at the first minibatch whose KL exceeds F, before that "
                         "minibatch's optimiser step; 0 (default): never.  --kl_early_stop 0.008 --scheduler none is rover_ppo.yaml as "
                         "skrl reads it, and rover_rpo.yaml is the same")
    ap.add_argument("--scheduler", choices=("kl_adaptive", "none"), default="kl_adaptive",
                    help="learning-rate scheduler stepped per epoch on the mean of the recorded KLs: skrl's KLAdaptiveRL (default), or "
                         "none (rover_ppo.yaml has its learning_rate_scheduler commented out)")
    ap.add_argument("--rewards_shaper_scale", type=float, default=None, metavar="F",
                    help="the agent files' rewards_shaper_scale: rewards are multiplied by F as they are recorded (default: off)")
    ap.add_argument("--time_limit_bootstrap", action="store_true",
                    help="skrl's time_limit_bootstrap: rewards += discount * value * truncated as they are recorded")
    ap.add_argument("--scan_noise", type=float, nargs=2, default=None, metavar=("N_MIN", "N_MAX"),
                    help="additive uniform noise on the height scan, the reference's Unoise (rover_env_cfg.py:23); default: none")
    ap.add_argument("--obs_backend", choices=("torch", "fused"), default="torch",
                    help="who applies --scan_noise: torch ops behind the step kernel, or one HIP launch with counter-based draws "
                         "(obs_post.ObsPost)")
    tracking.add_arguments(ap)
    return ap


class ScanNoise:
    """Additive uniform noise in the shape of ORBIT's AdditiveUniformNoiseCfg, without its func."""

    def __init__(self, n_min: float, n_max: float):
        self.n_min, self.n_max = n_min, n_max


def main():
    args = build_parser().parse_args()
    if args.kl_early_stop < 0:
        raise SystemExit("--kl_early_stop must be >= 0")
    scheduler = None if args.scheduler == "none" else args.scheduler
    skrl_loops = args.kl_early_stop > 0 or scheduler is None                    # the update follows skrl's loops, not the default ones
    shaped = args.rewards_shaper_scale is not None or args.time_limit_bootstrap
    shape_kw = dict(rewards_shaper_scale=args.rewards_shaper_scale, time_limit_bootstrap=args.time_limit_bootstrap, discount=GAMMA)
    upd_kw = dict(kl_early_stop=args.kl_early_stop, scheduler=scheduler) if skrl_loops else {}
    torch.manual_seed(42)
    dev = torch.device("cuda")
    n, Tn = args.num_envs, args.rollouts
    terrain = T.make_procedural_terrain((2048, 2048), seed=1234)
    terrain.make_spawns(2 * n)
    cfg = RoverEnvCfg(); cfg.scene.num_envs = n; cfg.terrain.kind = "custom"
    if args.scan_noise is not None:
        cfg.observations["height_scan"].noise = ScanNoise(*args.scan_noise)
        cfg.observation_post_backend = args.obs_backend
    env = RoverEnv(cfg, terrain=terrain)
    policy, value = Net(2, True).to(dev), Net(1, False).to(dev)
    opt = torch.optim.Adam(list(policy.parameters()) + list(value.parameters()), lr=1e-4)
    gamma, lam, clip, vclip, kl_thr = GAMMA, LAM, CLIP, VCLIP, KL_THR
    fused = None
    scaled = args.preprocess == "running"
    tscaled = None                              # the torch update behind the scalers
    if args.update == "fused":
        from isaac_rover_orbit_amd.ppo import FusedPPO
        from isaac_rover_orbit_amd.ppo_scaled import FusedScaledPPO
        fused = (FusedScaledPPO if scaled else FusedPPO)(policy.state_dict(), value.state_dict(), lr=1e-4)
    elif scaled:
        from isaac_rover_orbit_amd.ppo_scaled import TorchScaledPPO
        tscaled = TorchScaledPPO(policy, value, lr=1e-4, device=dev)
        if skrl_loops:
            from isaac_rover_orbit_amd.ppo_skrl import TorchSkrlPPO
            tscaled = TorchSkrlPPO(policy, value, lr=1e-4, device=dev)
    tskrl = None                                # the torch update on the raw rows with skrl's loops
    if fused is None and not scaled and skrl_loops:
        from isaac_rover_orbit_amd.ppo_skrl import TorchSkrlPPO
        tskrl = TorchSkrlPPO(policy, value, lr=1e-4, scalers=False, device=dev)
        opt = tskrl.opt
    # what the networks read and what the buffer stores of the critic, for the torch rollout glue
    if not scaled:
        standardise, unscale = (lambda x: x), (lambda v: v)
    elif fused is not None:
        standardise, unscale = fused.state_scaler.forward, (lambda v: fused.value_scaler.inverse(v.contiguous()))
    else:
        standardise = tscaled.state_preprocessor
        unscale = lambda v: tscaled.value_preprocessor(v, inverse=True)  # noqa: E731

    obs_buf = torch.empty(Tn, n, 965, device=dev)
    act_buf = torch.empty(Tn, n, 2, device=dev)
    logp_buf, val_buf, rew_buf = (torch.empty(Tn, n, device=dev) for _ in range(3))
    done_buf = torch.empty(Tn, n, device=dev)
    collector = None
    dev_scalers = None                          # device copies of the torch update's scalers, for the fused rollout
    if args.rollout == "fused":
        from isaac_rover_orbit_amd.rollout import RolloutCollector
        from isaac_rover_orbit_amd.rollout_scaled import ScaledRolloutCollector
        if fused is not None:                   # the trainer's networks and log-std by reference: always the current parameters
            if scaled:                          # ... and its two scaler blocks
                collector = ScaledRolloutCollector(fused.actor, fused.critic, fused.log_std, fused.state_scaler, fused.value_scaler,
                                                   n, Tn, seed=42)
            else:
                collector = RolloutCollector(fused.actor, fused.critic, fused.log_std, n, Tn, seed=42)
        else:                                   # re-packed networks are handed over at the top of every iteration
            nets = (RoverNet.from_state_dict(policy.state_dict(), final_act="tanh"),
                    RoverNet.from_state_dict(value.state_dict(), final_act="none"))
            if scaled:
                from isaac_rover_orbit_amd.scaler import DeviceScaler
                dev_scalers = (DeviceScaler(965, dev), DeviceScaler(1, dev))
                collector = ScaledRolloutCollector(*nets, policy.log_std_parameter.detach(), *dev_scalers, n, Tn, seed=42)
            else:
                collector = RolloutCollector(*nets, policy.log_std_parameter.detach(), n, Tn, seed=42)
        obs_buf, act_buf, logp_buf, val_buf = collector.obs, collector.actions, collector.logp, collector.val
        rew_buf, done_buf = collector.rew, collector.done
    # --track: skrl's curves on the device; the fused update's per-minibatch statistics feed skrl PPO's own scalars
    tracker = tracking.from_args(args, n, EPISODE_INFO_TAGS + (tracking.PPO_TAGS if fused is not None else ()), dev)
    obs, _ = env.reset()
    o = obs["policy"] if collector is not None else torch.nan_to_num(obs["policy"], neginf=0.0)
    out = open(args.out, "w") if args.out else None
    for it in range(args.iterations):
        t0 = time.perf_counter()
        # ---- rollout on the fused kernels
        if fused is None:
            actor = RoverNet.from_state_dict(policy.state_dict(), final_act="tanh")
            critic = RoverNet.from_state_dict(value.state_dict(), final_act="none")
            log_std = policy.log_std_parameter.detach().clamp(-20.0, 2.0)
        else:                                   # the trainer's own parameters: nothing to re-pack
            actor, critic = fused.actor, fused.critic
            log_std = fused.log_std.clamp(-20.0, 2.0)
        std = log_std.exp()
        ep_count = torch.zeros((), device=dev); ep_stats = torch.zeros(4, device=dev)
        if collector is not None:
            collector.actor, collector.critic = actor, critic
            if dev_scalers is not None:         # the torch scalers' statistics after the last update
                dev_scalers[0].load_state_dict(tscaled.state_preprocessor.state_dict())
                dev_scalers[1].load_state_dict(tscaled.value_preprocessor.state_dict())
        for t in range(Tn):
            if collector is not None:           # the raw rows go in; slot t of every buffer comes out
                obs, rew, term, trunc, info = env.step(collector.act(t, o))
                o = obs["policy"]
                collector.record(t, rew, term, trunc, **(shape_kw if shaped else {}))
                lv = env.episode_log_vector
                ep_count += lv[13]; ep_stats += torch.where(lv[13] > 0, lv[7:11], torch.zeros_like(lv[7:11]))
                if tracker is not None:         # the env's raw reward; lv is behind the env's own log reduction
                    tracker.step(rew, term, trunc)
                    tracker.track_vector(EPISODE_INFO_TAGS, lv)
                    tracker.post_interaction(it * Tn + t)
                continue
            s = standardise(o)                  # the buffer keeps the raw rows; the networks read the standardised ones
            mean = actor(s)
            a = mean + std * torch.randn_like(mean)
            logp_buf[t] = (-0.5 * ((a - mean) / std) ** 2 - log_std - 0.9189385332).sum(1)
            val_buf[t] = unscale(critic(s)).squeeze(1)
            obs_buf[t], act_buf[t] = o, a
            obs, rew, term, trunc, info = env.step(a.clamp(-1.0, 1.0))      # clip_actions (models.py:66)
            o = torch.nan_to_num(obs["policy"], neginf=0.0)
            if tracker is not None:
                tracker.step(rew, term, trunc)
                tracker.track_vector(EPISODE_INFO_TAGS, env.episode_log_vector)
                tracker.post_interaction(it * Tn + t)
            if shaped:
                from isaac_rover_orbit_amd.ppo_skrl import shape_rewards
                rew = shape_rewards(rew, val_buf[t], trunc, 1.0 if args.rewards_shaper_scale is None else args.rewards_shaper_scale,
                                    GAMMA, args.time_limit_bootstrap)
            rew_buf[t], done_buf[t] = rew, (term | trunc).float()
            lv = env.episode_log_vector
            ep_count += lv[13]; ep_stats += torch.where(lv[13] > 0, lv[7:11], torch.zeros_like(lv[7:11]))
        torch.cuda.synchronize(); t_roll = time.perf_counter() - t0
        if fused is not None:
            # ---- GAE and the PPO update on the fused HIP kernels (isaac_rover_orbit_amd.ppo)
            with torch.no_grad():
                last_v = collector.last_value(o) if collector is not None else unscale(critic(standardise(o))).squeeze(1)
                adv, ret = fused.gae(rew_buf, done_buf, val_buf, last_v)
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            if scaled:                          # skrl PPO._update: the value scaler trains on the values, then on the returns
                val_s, ret_s = fused.standardize_values(val_buf, ret)
                kls, _ = fused.update(obs_buf, act_buf, logp_buf, val_s, ret_s, adv, **upd_kw)
            else:
                kls, _ = fused.update(obs_buf, act_buf, logp_buf, val_buf, ret, adv, **upd_kw)
            kl_mean = kls[-1]
            last = fused.last_update
            if tracker is not None:
                tracking.track_ppo_update(tracker, fused)
        else:
            # ---- GAE (skrl PPO: bootstraps through time-outs like the reference's config)
            with torch.no_grad():
                last_v = collector.last_value(o) if collector is not None else unscale(critic(standardise(o))).squeeze(1)
                adv = torch.zeros_like(rew_buf); gae = torch.zeros(n, device=dev)
                for t in reversed(range(Tn)):
                    nv = last_v if t == Tn - 1 else val_buf[t + 1]
                    nd = 1.0 - done_buf[t]
                    delta = rew_buf[t] + gamma * nv * nd - val_buf[t]
                    gae = delta + gamma * lam * nd * gae
                    adv[t] = gae
                ret = adv + val_buf
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            # ---- PPO update (torch autograd)
            B = Tn * n
            fo, fa, flp, fv, fr, fadv = (x.reshape(B, *x.shape[2:]) for x in (obs_buf, act_buf, logp_buf, val_buf, ret, adv))
            kl_mean = 0.0
            last = None
            if scaled:                          # the same update behind the two scalers (ppo_scaled.TorchScaledPPO)
                val_s, ret_s = tscaled.standardize_values(fv, fr)
                kl_mean = tscaled.update(fo, fa, flp, val_s, ret_s, fadv, **upd_kw)[0][-1]
                last = getattr(tscaled, "last_update", None)
            elif tskrl is not None:             # skrl's loops on the raw rows (ppo_skrl.TorchSkrlPPO)
                kl_mean = tskrl.update(fo, fa, flp, fv, fr, fadv, **upd_kw)[0][-1]
                last = tskrl.last_update
            for epoch in range(0 if scaled or tskrl is not None else 4):   # the unscaled update, as before
                perm = torch.randperm(B, device=dev)
                kls = []
                for mb in perm.chunk(60):
                    loss, kl = ppo_loss(policy, value, fo[mb], fa[mb], flp[mb], fv[mb], fr[mb], fadv[mb], clip, vclip)
                    kls.append(kl)
                    opt.zero_grad(set_to_none=True)
                    loss.backward()
                    nn.utils.clip_grad_norm_(list(policy.parameters()) + list(value.parameters()), 0.5)
                    opt.step()
                kl_mean = torch.stack(kls).mean().item()
                lr = opt.param_groups[0]["lr"]                     # KLAdaptiveRL
                if kl_mean > 2 * kl_thr: lr = max(lr / 1.5, 1e-6)
                elif kl_mean < 0.5 * kl_thr: lr = min(lr * 1.5, 1e-2)
                for g in opt.param_groups: g["lr"] = lr
        torch.cuda.synchronize()
        st = {"iteration": it, "mean_step_reward": rew_buf.mean().item(), "episodes": ep_count.item(),
              "time_out": ep_stats[0].item(), "success": ep_stats[1].item(), "far": ep_stats[2].item(),
              "collision": ep_stats[3].item(), "kl": kl_mean,
              "lr": fused.lr if fused is not None else tscaled.lr if tscaled is not None else opt.param_groups[0]["lr"],
              "recorded": last["recorded"] if last else [60] * 4, "stopped": last["stopped"] if last else [False] * 4,
              "rollout_s": t_roll, "rollout_env_steps_per_s": Tn * n / t_roll, "iteration_s": time.perf_counter() - t0}
        print(json.dumps(st), flush=True)
        if out:
            out.write(json.dumps(st) + "\n"); out.flush()
    if args.save:
        torch.save(fused.state_dict() if fused is not None else tscaled.state_dict() if tscaled is not None
                   else {"policy": policy.state_dict(), "value": value.state_dict()}, args.save)
    env.close()


if __name__ == "__main__":
    main()
