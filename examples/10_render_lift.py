#!/usr/bin/env python3
"""Look at FrankaCubeLift-v0: render frames of a random or checkpointed policy with the rgb_array viewer
and write them to an .npz (``frames`` (T, H, W, 3) uint8, ``object_id`` (T, H, W) int32 of the same frames).

    python examples/10_render_lift.py --num_envs 16 --frames 8 --every 10 --out lift_frames.npz
    python examples/10_render_lift.py --checkpoint lift_ppo.pt --env 3 --out lift_env3.npz      # a checkpoint of 05_train_lift.py

``--env k`` places the camera relative to env k's origin (ORBIT's ViewerCfg origin_type "env"); without it the camera is the
reference's world view, eye (-6, -6, 3.5).  The reference's own scripts get the same frames through ``--video``
(``gym.make(..., viewport=True)`` + ``gymnasium.wrappers.RecordVideo``).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isaac_rover_orbit_amd import lift_ppo as LP  # noqa: E402
from isaac_rover_orbit_amd.cfg import ViewerCfg  # noqa: E402
from isaac_rover_orbit_amd.envs.lift_env import FrankaCubeLiftEnv, LiftEnvCfg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=16)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--every", type=int, default=10, help="env steps between two frames")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--checkpoint", default=None, help="skrl-style checkpoint of examples/05_train_lift.py --save (default: random actions)")
    ap.add_argument("--env", type=int, default=None, help="follow this env: eye (1.8, -1.5, 1.0) from its origin, looking at its table")
    ap.add_argument("--resolution", type=int, nargs=2, default=(640, 360), metavar=("W", "H"))
    ap.add_argument("--out", default="lift_frames.npz")
    args = ap.parse_args()
    cfg = LiftEnvCfg()
    cfg.scene.num_envs, cfg.seed = args.num_envs, args.seed
    if args.env is None:
        cfg.viewer = ViewerCfg(eye=(-6.0, -6.0, 3.5), resolution=tuple(args.resolution))
    else:
        cfg.viewer = ViewerCfg(eye=(1.8, -1.5, 1.0), lookat=(0.4, 0.0, 0.3), resolution=tuple(args.resolution), origin_type="env",
                               env_index=args.env)
    env = FrankaCubeLiftEnv(cfg, render_mode="rgb_array")
    act = None
    if args.checkpoint:
        ck = torch.load(args.checkpoint, map_location=env.device)
        actor = LP.lift_net(ck["policy"])
        scaler = LP.RunningStandardScaler(LP.OBS_DIM, device=env.device)
        if "state_preprocessor" in ck:
            scaler.load_state_dict(ck["state_preprocessor"])
        act = lambda o: actor(scaler(o))                                                          # noqa: E731  (the policy's mean)
    g = torch.Generator(device=env.device).manual_seed(args.seed)
    obs, _ = env.reset()
    frames, ids = [], []
    with torch.no_grad():
        for f in range(args.frames):
            rgba, _, oid = env.render_frame(object_id=True)
            frames.append(rgba[..., :3].cpu().numpy())
            ids.append(oid.cpu().numpy())
            for _ in range(args.every):
                a = act(obs["policy"]) if act else torch.rand(args.num_envs, 8, device=env.device, generator=g) * 2 - 1
                obs, *_ = env.step(a)
    np.savez_compressed(args.out, frames=np.stack(frames), object_id=np.stack(ids))
    drawn = np.stack(ids) >= 2
    print(f"wrote {args.out}: {len(frames)} frames of {args.resolution[0]} x {args.resolution[1]}, {drawn.mean() * 100:.1f} % of the pixels on an env")
    env.close()


if __name__ == "__main__":
    main()
