#!/usr/bin/env python3
"""What ORBIT's observation post-processing costs beside the step kernel, per backend, and the depth camera's noise pass beside
the render it follows.

    python tools/obs_post_bench.py --trace --out profiles/obs_post_bench.json

Workload: 4096 envs on the config-2 terrain (procedural 2048^2 at 0.05 m, sigma_z 0.15 m, seed 1234, 400 rocks), the stock term
table plus uniform noise and a clip on the height scan.  Three envs step the same actions: ``observation_post_backend = "torch"``
(torch ops behind the step kernel), ``"fused"`` (one ``rover_obs_post_apply`` launch) and one without post-processing.  After
``--preroll`` untimed steps each (episodes of mixed age, the device at its sustained clocks) the three alternate in one process:
a round is ``--steps`` back-to-back ``env.step`` calls per env under a host clock, ending in one device synchronise; the figure is
the median over ``--reps`` rounds with min .. max.  The depth pass is timed the same way on a 160 x 90 camera: the render alone
against the render followed by the noise + clip launch.

``--trace``: before this process opens the GPU, child processes run the fused env (and the noisy camera) alone under
``rocprofv3 --kernel-trace --stats`` (no counters in that run); the kernels' average device times come from there.

Traffic floors (bytes that must move, read + written): observation rows 4096 x 965 x 4 B x 2 = 31.6 MB per step (the scan's 961
columns alone: 31.5 MB); depth images 4096 x 14400 x 4 B x 2 = 471.9 MB per pass (236 MB each way).
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Unoise:
    def __init__(self, n_min, n_max):
        self.n_min, self.n_max = n_min, n_max


class Gnoise:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std


def make_terrain(n):
    from isaac_rover_orbit_amd import terrain as T
    ter = T.make_procedural_terrain((2048, 2048), seed=1234, sigma_z=0.15, n_rocks=400)
    ter.make_spawns(2 * n, seed=41)
    return ter


def make_env(ter, n, backend, camera=None):
    """``backend``: "torch" / "fused" (noise + clip on the height scan) or None (the stock table)."""
    from isaac_rover_orbit_amd.cfg import RoverEnvCfg
    from isaac_rover_orbit_amd.envs import RoverEnv
    cfg = RoverEnvCfg()
    cfg.scene.num_envs, cfg.terrain.kind = n, "custom"
    if backend is not None:
        hs = cfg.observations["height_scan"]
        hs.noise, hs.clip = Unoise(-0.02, 0.03), (-1.0, 1.0)
        cfg.observation_post_backend = backend
    cfg.camera = camera
    return RoverEnv(cfg, terrain=ter)


def noisy_camera():
    from isaac_rover_orbit_amd.cfg import CameraCfg
    return CameraCfg(noise=Gnoise(0.0, 0.02), clip=(0.0, 10.0))


def summary(xs, per=1):
    return {"median_us": 1e6 * statistics.median(xs) / per, "min_us": 1e6 * min(xs) / per, "max_us": 1e6 * max(xs) / per, "rounds": len(xs)}


def child(args):
    """The traced workload: nothing but the launches whose kernels are wanted."""
    import torch
    ter = make_terrain(args.envs)
    a = torch.zeros(args.envs, 2, device="cuda")
    if args.child == "rows":
        env = make_env(ter, args.envs, "fused")
        env.reset()
        for _ in range(args.steps):
            env.step(a)
    else:
        env = make_env(ter, args.envs, None, camera=noisy_camera())
        env.reset()
        for _ in range(args.steps):
            env.render_depth()
    torch.cuda.synchronize()
    env.close()


def trace(args, what, steps):
    """{kernel name: calls, average_us} of a child run under the kernel trace; only this tree's env / camera / post kernels."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return {"skipped": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--child", what, "--steps", str(steps), "--envs", str(args.envs)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            return {"skipped": f"the traced child ended with {r.returncode}", "stderr": r.stderr[-400:]}
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                rows += list(csv.DictReader(f))
    out = {}
    for r in rows:
        name = r.get("Name", "").replace("(anonymous namespace)::", "").replace("void ", "")
        if any(k in name for k in ("obs_post_kernel", "rover_step", "rover_scan", "camera")):
            out[name.split("(")[0]] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3}
    return out or {"skipped": "no kernel of interest in the trace"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--preroll", type=int, default=1500)
    ap.add_argument("--steps", type=int, default=200, help="back-to-back steps per round")
    ap.add_argument("--reps", type=int, default=9, help="rounds per env; the envs alternate")
    ap.add_argument("--renders", type=int, default=20, help="renders per round of the depth pass")
    ap.add_argument("--no-depth", action="store_true")
    ap.add_argument("--trace", action="store_true", help="also the kernels' device times from traced child processes")
    ap.add_argument("--child", choices=("rows", "depth"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    traces = None
    if args.trace:                                             # before this process opens the GPU
        traces = {"rows": trace(args, "rows", 200)}
        if not args.no_depth:
            traces["depth"] = trace(args, "depth", 20)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("obs_post_bench.py measures on a ROCm GPU; none is available")
    n = args.envs
    ter = make_terrain(n)
    envs = {"torch": make_env(ter, n, "torch"), "fused": make_env(ter, n, "fused"), "plain": make_env(ter, n, None)}
    g = torch.Generator(device="cuda").manual_seed(0)
    actions = torch.rand(256, n, 2, device="cuda", generator=g) * 2 - 1
    for env in envs.values():
        env.reset()
        for k in range(args.preroll):
            env.step(actions[(k * 7) % 256])
    torch.cuda.synchronize()
    times = {k: [] for k in envs}
    for _ in range(args.reps):
        for name, env in envs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(args.steps):
                env.step(actions[k % 256])
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    res = {"envs": n, "preroll": args.preroll, "steps_per_round": args.steps,
           "table": "stock + height_scan noise U(-0.02, 0.03), clip (-1, 1)",
           "step": {k: summary(v, args.steps) for k, v in times.items()},
           "row_traffic_floor_MB": n * 965 * 4 * 2 / 1e6, "kernel_names": list(envs["fused"].kernel_names())}
    med = {k: res["step"][k]["median_us"] for k in envs}
    res["post_cost_us"] = {"torch": med["torch"] - med["plain"], "fused": med["fused"] - med["plain"]}
    res["fused_closer_to_plain_than_to_torch"] = (med["fused"] - med["plain"]) < (med["torch"] - med["fused"])
    for env in envs.values():
        env.close()
    del envs
    if not args.no_depth:
        from isaac_rover_orbit_amd.obs_post import DEPTH_TAG, ObsPost, image_segments
        cam = noisy_camera()
        env = make_env(ter, n, None, camera=cam)
        env.reset()
        post, env.sensors.depth_post = env.sensors.depth_post, None           # the launches are made by hand below
        assert isinstance(post, ObsPost) and post.tag == DEPTH_TAG and len(image_segments(cam)) == 1
        buf = torch.empty(n, cam.height, cam.width, device="cuda")

        def render():
            env.sensors.render_into(buf)

        def render_post():
            env.sensors.render_into(buf)
            post.apply(buf, 0)

        for fn in (render, render_post):
            for _ in range(5):
                fn()
        dt = {"render": [], "render_noise_clip": []}
        for _ in range(args.reps):
            for name, fn in (("render", render), ("render_noise_clip", render_post)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _k in range(args.renders):
                    fn()
                torch.cuda.synchronize()
                dt[name].append(time.perf_counter() - t0)
        res["depth"] = {k: summary(v, args.renders) for k, v in dt.items()}
        res["depth"]["pass_cost_us"] = res["depth"]["render_noise_clip"]["median_us"] - res["depth"]["render"]["median_us"]
        res["depth"]["image_traffic_floor_MB"] = n * cam.height * cam.width * 4 * 2 / 1e6
        env.close()
    if traces is not None:
        res["kernel_trace"] = traces
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
