#!/usr/bin/env python3
"""DAgger on the HIP-backed rover env: distil a privileged teacher (a PPO policy trained on the 961-ray height scan, e.g. by
examples/04_train_ppo.py) into a student that drives from the on-board camera's 31 x 31 depth image.  This is what the reference's
``RoverEnvCamera`` is for ("collecting camera data for Learning By Cheating"); the reference has no trainer for it.

At 31 x 31 the image has 961 pixels, the width of the height scan, so the student is the reference's policy network on a 965-wide row
whose scan columns hold depth (``isaac_rover_orbit_amd.dagger``).  Every env step: the teacher labels the state, env i is driven by the
teacher with probability beta and by the student otherwise, the student's row and the label go into the dataset (a
``td3.ReplayMemory``), and one imitation step runs on a batch drawn from it.  ``--update fused`` runs all of that but ``env.step`` as HIP
kernels (``DAggerCollector`` + ``FusedDAgger``); ``--update torch`` is the specification on the same device.

``--student conv`` keeps the camera at the reference's 160 x 90 and puts a small learned convolutional stem in front of the same
network (``isaac_rover_orbit_amd.dagger_conv``): the images go into an ``ImageRing`` beside the dataset and stem and network train end
to end.  The default ``--student mlp31`` is the 31 x 31 student described above.

beta follows ``beta0 * beta_decay ** step``: ``--beta0 1 --beta_decay 1`` is behaviour cloning, ``--beta0 0`` the pure student.

    python examples/11_distil_student.py --teacher ppo.pt --num_envs 256 --steps 50 --update fused --save student.pt
    python examples/11_distil_student.py --eval student.pt --num_envs 256 --steps 750
    python examples/11_distil_student.py --teacher ppo.pt --student conv --num_envs 256 --batch_size 1024 --update fused --save conv.pt
    python examples/11_distil_student.py --eval conv.pt --student conv --num_envs 256 --steps 750

``--eval`` drives closed loop from the student's own rows and prints the termination tallies, as examples/03_eval_policy.py does.  No
claim is made about how well a student trained this way drives.
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
from isaac_rover_orbit_amd import dagger, dagger_conv  # noqa: E402
from isaac_rover_orbit_amd import terrain as T  # noqa: E402
from isaac_rover_orbit_amd import tracker as tracking  # noqa: E402
from isaac_rover_orbit_amd.cfg import RoverEnvCfg  # noqa: E402
from isaac_rover_orbit_amd.envs import RoverEnv  # noqa: E402
from isaac_rover_orbit_amd.envs.rover_env import LOG_KEYS  # noqa: E402
from isaac_rover_orbit_amd.policy import RoverNet  # noqa: E402
from isaac_rover_orbit_amd.td3 import ReplayMemory  # noqa: E402

_spec = importlib.util.spec_from_file_location("train_ppo_example", os.path.join(ROOT, "examples", "04_train_ppo.py"))
ppo_example = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ppo_example)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--teacher", default=None, help="skrl-style checkpoint whose 'policy' entry is the teacher (examples/04 --save)")
    ap.add_argument("--eval", default=None, metavar="CKPT", help="evaluate this student checkpoint closed loop instead of training")
    ap.add_argument("--update", choices=("torch", "fused"), default="torch",
                    help="collector and update: the torch specification or the fused HIP kernels")
    ap.add_argument("--student", choices=("mlp31", "conv"), default="mlp31",
                    help="mlp31: a 31 x 31 camera straight into the network; conv: the 160 x 90 camera through a learned stem")
    ap.add_argument("--num_envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--beta0", type=float, default=1.0)
    ap.add_argument("--beta_decay", type=float, default=0.95)
    ap.add_argument("--batch_size", type=int, default=4096)
    ap.add_argument("--memory_size", type=int, default=None, help="dataset slots (default: enough for 2 x batch_size rows, at least 16)")
    ap.add_argument("--learning_rate", type=float, default=dagger.HPARAMS["learning_rate"])
    ap.add_argument("--grad_norm_clip", type=float, default=dagger.HPARAMS["grad_norm_clip"])
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--log_every", type=int, default=10, help="env steps per logged line (the fused path syncs only then)")
    ap.add_argument("--save", default=None, metavar="PATH", help="write {'policy': student state_dict}, loadable by --eval and RoverNet")
    ap.add_argument("--depth_noise_std", type=float, default=None, metavar="S",
                    help="Gaussian sensor noise of standard deviation S (m) on the depth image the student sees (default: none)")
    ap.add_argument("--depth_clip_max", type=float, default=None, metavar="M",
                    help="clip the depth image to [0, M] m after the noise: misses (+inf) become M (default: no clip)")
    # a depth sensor model between the render and the noise / clip above (CameraCfg.sensor, depth_sensor.py); none by default
    ap.add_argument("--depth_range", type=float, nargs=2, default=None, metavar=("MIN", "MAX"),
                    help="the sensor's working range (m): depths outside it, misses included, read --depth_invalid")
    ap.add_argument("--depth_sigma", type=float, nargs=3, default=None, metavar=("S0", "S1", "S2"),
                    help="axial noise of standard deviation S0 + S1 z + S2 z^2 (m) at depth z")
    ap.add_argument("--depth_dropout", type=float, nargs=2, default=None, metavar=("P", "P_EDGE"),
                    help="probability that a pixel loses its data, off and on a depth edge")
    ap.add_argument("--depth_disparity_step", type=float, default=None, metavar="PX", help="quantise the disparity in steps of PX pixels")
    ap.add_argument("--depth_baseline", type=float, default=None, metavar="M", help="stereo baseline (m) of the disparity steps (default 0.05)")
    ap.add_argument("--depth_invalid", type=float, default=None, metavar="V", help="what a pixel without data reads (default 0)")
    tracking.add_arguments(ap)
    return ap


def sensor_cfg(args):
    """``CameraCfg.sensor`` of the --depth_range / _sigma / _dropout / _disparity_step / _baseline / _invalid flags; None without any."""
    from isaac_rover_orbit_amd.cfg import DepthSensorCfg
    given = (args.depth_range, args.depth_sigma, args.depth_dropout, args.depth_disparity_step, args.depth_baseline, args.depth_invalid)
    if all(v is None for v in given):
        return None
    s = DepthSensorCfg()
    if args.depth_range is not None:
        s.range_min, s.range_max = args.depth_range
    if args.depth_sigma is not None:
        s.sigma = tuple(args.depth_sigma)
    if args.depth_dropout is not None:
        s.p_drop, s.p_edge = args.depth_dropout
    if args.depth_disparity_step is not None:
        s.disparity_step = args.depth_disparity_step
    if args.depth_baseline is not None:
        s.baseline = args.depth_baseline
    if args.depth_invalid is not None:
        s.invalid_value = args.depth_invalid
    return s


class DepthNoise:
    """Zero-mean Gaussian noise in the shape of ORBIT's AdditiveGaussianNoiseCfg, without its func."""

    def __init__(self, std: float):
        self.mean, self.std = 0.0, std


def make_env(n: int, student: str = "mlp31", depth_noise_std: float | None = None, depth_clip_max: float | None = None, sensor=None):
    terrain = T.make_procedural_terrain((2048, 2048), seed=1234)
    terrain.make_spawns(2 * n)
    cfg = RoverEnvCfg(); cfg.scene.num_envs = n; cfg.terrain.kind = "custom"
    cfg.camera = dagger_conv.student_camera_cfg() if student == "conv" else dagger.student_camera_cfg()
    cfg.camera.sensor = sensor
    if depth_noise_std is not None:
        cfg.camera.noise = DepthNoise(depth_noise_std)
    if depth_clip_max is not None:
        cfg.camera.clip = (0.0, depth_clip_max)
    return cfg, RoverEnv(cfg, terrain=terrain)


def evaluate(args):
    """examples/03_eval_policy.py's loop with the student's rows in place of the env's."""
    _, env = make_env(args.num_envs, args.student, args.depth_noise_std, args.depth_clip_max, sensor_cfg(args))
    if args.student == "conv":
        act = dagger_conv.ConvStudent.from_checkpoint(args.eval).act
    else:
        actor = RoverNet.from_checkpoint(args.eval, role="policy")
        rows = torch.empty(args.num_envs, 965, device="cuda")

        def act(obs, depth):
            return actor(dagger.fused_student_rows(depth, obs["policy"], out=rows))
    obs, _ = env.reset()
    counts, episodes = torch.zeros(4), 0.0
    for _ in range(args.steps):
        obs, rew, terminated, truncated, info = env.step(act(obs, env.extras["depth"]))
        log = env.episode_log_vector.cpu()
        if log[13] > 0:
            episodes += float(log[13])
            counts += log[7:11]
    print(f"episodes finished: {episodes:.0f}; terminations (time_out, success, far, collision): {counts.tolist()}")
    env.close()


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.eval:
        return evaluate(args)
    if not args.teacher:
        ap.error("--teacher CKPT is required to train (or --eval CKPT to evaluate)")
    torch.manual_seed(args.seed)
    dev = torch.device("cuda")
    n = args.num_envs
    M = args.memory_size or max(16, -(-2 * args.batch_size // n))
    cfg, env = make_env(n, args.student, args.depth_noise_std, args.depth_clip_max, sensor_cfg(args))
    teacher_sd = torch.load(args.teacher, map_location="cpu", weights_only=False)["policy"]
    memory = ReplayMemory(M, n, device=dev)
    student = ppo_example.Net(2, True).to(dev)
    hp = dict(learning_rate=args.learning_rate, grad_norm_clip=args.grad_norm_clip)
    images = None
    if args.student == "conv":
        # the images of every slot of the dataset: (M + 1) x n x 57.6 KB beside the memory
        images = dagger_conv.ImageRing(M, n, device=dev)
        if args.update == "fused":
            trainer = dagger_conv.FusedConvDAgger(student.state_dict(), seed=args.seed, **hp)
            collector = dagger_conv.ConvDAggerCollector(RoverNet.from_state_dict(teacher_sd, final_act="tanh"), trainer, memory, images,
                                                        seed=args.seed, env_id_offset=cfg.env_id_offset)
        else:
            teacher = ppo_example.Net(2, True).to(dev)
            teacher.load_state_dict(teacher_sd, strict=False)
            stem = dagger_conv.ConvStem.seeded(args.seed).to(dev)
            trainer = dagger_conv.TorchConvDAgger(student, stem, **hp)
            collector = dagger_conv.TorchConvDAggerCollector(teacher, student, stem, memory, images, seed=args.seed,
                                                             env_id_offset=cfg.env_id_offset)
    elif args.update == "fused":
        trainer = dagger.FusedDAgger(student.state_dict(), **hp)
        collector = dagger.DAggerCollector(RoverNet.from_state_dict(teacher_sd, final_act="tanh"), trainer.actor, memory, seed=args.seed,
                                           env_id_offset=cfg.env_id_offset)
    else:
        teacher = ppo_example.Net(2, True).to(dev)
        teacher.load_state_dict(teacher_sd, strict=False)
        trainer = dagger.TorchDAgger(student, **hp)
        collector = dagger.TorchDAggerCollector(teacher, student, memory, seed=args.seed, env_id_offset=cfg.env_id_offset)
    EPISODE_INFO_TAGS = tracking.episode_info_tags(LOG_KEYS)
    tracker = tracking.from_args(args, n, EPISODE_INFO_TAGS, dev)      # --track: the reward and episode curves only
    obs, _ = env.reset()
    collector.begin(obs, env.extras["depth"])
    t_log, steps_log, last = time.perf_counter(), 0, {}
    for step in range(args.steps):
        beta = args.beta0 * args.beta_decay ** step
        obs, rew, term, trunc, info = env.step(collector.act(beta))
        idx = collector.record(obs, env.extras["depth"], rew, term, batch_size=args.batch_size)
        if tracker is not None:
            tracker.step(rew, term, trunc)
            tracker.track_vector(EPISODE_INFO_TAGS, env.episode_log_vector)
            tracker.post_interaction(step)
        out = trainer.update(memory, idx) if images is None else trainer.update(memory, images, idx)
        steps_log += 1
        if (step + 1) % args.log_every == 0 or step + 1 == args.steps:
            if args.update == "fused":
                s = trainer.stats()
                last = {k: s[k] for k in ("loss", "grad_norm", "steps", "bad_index")}
            else:
                last = {k: out[k] for k in ("loss", "grad_norm")}
            torch.cuda.synchronize()
            dt = time.perf_counter() - t_log
            print(json.dumps({"timestep": step + 1, "beta": beta, "dataset_rows": len(memory), **last,
                              "env_steps_per_s": steps_log * n / dt}), flush=True)
            t_log, steps_log = time.perf_counter(), 0
    if args.save:
        torch.save(trainer.checkpoint(), args.save)
    env.close()


if __name__ == "__main__":
    main()
