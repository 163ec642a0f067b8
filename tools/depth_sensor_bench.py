#!/usr/bin/env python3
"""What the depth sensor model costs behind the render it follows, beside the camera's noise + clip pass.

    python tools/depth_sensor_bench.py --trace --out profiles/depth_sensor_bench.json

Workload: 4096 envs on the config-2 terrain (procedural 2048^2 at 0.05 m, sigma_z 0.15 m, seed 1234, 400 rocks) with the 160 x 90
camera, after ``--preroll`` untimed steps (episodes of mixed age, the device at its sustained clocks).  Three items alternate in one
process: ``render_depth()``'s launches alone, the render followed by ``rover_depth_sensor_apply`` with every stage on (range,
edge-aware dropout, axial noise, disparity steps, valid counts), and the render followed by ``CameraCfg.noise`` Gaussian + clip
(``rover_obs_post_apply``, the yardstick: it moves the same bytes).  A round is ``--renders`` back-to-back calls under a host clock,
ending in one device synchronise; the figure is the median over ``--reps`` rounds with min .. max.

``--trace``: before this process opens the GPU, one child process runs the sensor camera alone under ``rocprofv3 --kernel-trace
--stats`` (no counters in that run); the kernels' average device times come from there.

Traffic floor (bytes that must move, read + written): 4096 x 14400 x 4 B x 2 = 471.9 MB per pass (236 MB each way).
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


class Gnoise:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std


def make_terrain(n):
    from isaac_rover_orbit_amd import terrain as T
    ter = T.make_procedural_terrain((2048, 2048), seed=1234, sigma_z=0.15, n_rocks=400)
    ter.make_spawns(2 * n, seed=41)
    return ter


def sensor_cfg():
    """Every stage on."""
    from isaac_rover_orbit_amd.cfg import DepthSensorCfg
    return DepthSensorCfg(range_min=0.3, range_max=8.0, sigma=(0.001, 0.0005, 0.002), p_drop=0.01, p_edge=0.4, disparity_step=0.125)


def make_env(ter, n, camera):
    from isaac_rover_orbit_amd.cfg import RoverEnvCfg
    from isaac_rover_orbit_amd.envs import RoverEnv
    cfg = RoverEnvCfg()
    cfg.scene.num_envs, cfg.terrain.kind = n, "custom"
    cfg.camera = camera
    return RoverEnv(cfg, terrain=ter)


def summary(xs, per=1):
    return {"median_us": 1e6 * statistics.median(xs) / per, "min_us": 1e6 * min(xs) / per, "max_us": 1e6 * max(xs) / per, "rounds": len(xs)}


def child(args):
    """The traced workload: nothing but the launches whose kernels are wanted."""
    import torch
    from isaac_rover_orbit_amd.cfg import CameraCfg
    env = make_env(make_terrain(args.envs), args.envs, CameraCfg(sensor=sensor_cfg(), noise=Gnoise(0.0, 0.02), clip=(0.0, 10.0)))
    env.reset()
    for _ in range(args.renders):
        env.render_depth()
    torch.cuda.synchronize()
    env.close()


def trace(args):
    """{kernel name: calls, average_us} of the child run under the kernel trace; only the camera's and the two passes' kernels."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return {"skipped": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--renders", str(args.renders), "--envs", str(args.envs)]
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
        if any(k in name for k in ("depth_sensor_kernel", "obs_post_kernel", "camera")):
            out[name.split("(")[0]] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3}
    return out or {"skipped": "no kernel of interest in the trace"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--preroll", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=9, help="rounds per item; the items alternate")
    ap.add_argument("--renders", type=int, default=20, help="renders per round")
    ap.add_argument("--trace", action="store_true", help="also the kernels' device times from a traced child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    traces = trace(args) if args.trace else None                 # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("depth_sensor_bench.py measures on a ROCm GPU; none is available")
    from isaac_rover_orbit_amd.cfg import CameraCfg
    from isaac_rover_orbit_amd.depth_sensor import DepthSensor
    from isaac_rover_orbit_amd.obs_post import ObsPost
    n = args.envs
    cam = CameraCfg(sensor=sensor_cfg(), noise=Gnoise(0.0, 0.02), clip=(0.0, 10.0))
    env = make_env(make_terrain(n), n, cam)
    g = torch.Generator(device="cuda").manual_seed(0)
    actions = torch.rand(256, n, 2, device="cuda", generator=g) * 2 - 1
    env.reset()
    cam.every_n_steps, env.sensors.camera_every = 1 << 30, 1 << 30      # the pre-roll renders nothing
    for k in range(args.preroll):
        env.step(actions[(k * 7) % 256])
    sensor, post = env.sensors.depth_sensor, env.sensors.depth_post
    env.sensors.depth_sensor = env.sensors.depth_post = None                   # the launches are made by hand below
    assert isinstance(sensor, DepthSensor) and isinstance(post, ObsPost)
    buf = torch.empty(n, cam.height, cam.width, device="cuda")
    valid = torch.empty(n, dtype=torch.int32, device="cuda")

    def render():
        env.sensors.render_into(buf)

    def render_sensor():
        env.sensors.render_into(buf)
        sensor.apply(buf, 0, valid_out=valid)

    def render_noise_clip():
        env.sensors.render_into(buf)
        post.apply(buf, 0)

    items = (("render", render), ("render_sensor", render_sensor), ("render_noise_clip", render_noise_clip))
    for _, fn in items:
        for _ in range(5):
            fn()
    render_sensor()
    torch.cuda.synchronize()
    valid_share = float(valid.double().mean()) / (cam.height * cam.width)
    dt = {name: [] for name, _ in items}
    for _ in range(args.reps):
        for name, fn in items:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _k in range(args.renders):
                fn()
            torch.cuda.synchronize()
            dt[name].append(time.perf_counter() - t0)
    res = {"envs": n, "preroll": args.preroll, "renders_per_round": args.renders, "image": [cam.height, cam.width],
           "sensor": "range (0.3, 8), sigma (0.001, 0.0005, 0.002), p_drop 0.01, p_edge 0.4, disparity_step 0.125, valid_out",
           "valid_share": valid_share}
    res.update({k: summary(v, args.renders) for k, v in dt.items()})
    res["sensor_pass_cost_us"] = res["render_sensor"]["median_us"] - res["render"]["median_us"]
    res["noise_clip_pass_cost_us"] = res["render_noise_clip"]["median_us"] - res["render"]["median_us"]
    res["sensor_over_noise_clip"] = res["sensor_pass_cost_us"] / res["noise_clip_pass_cost_us"]
    res["image_traffic_floor_MB"] = n * cam.height * cam.width * 4 * 2 / 1e6
    env.close()
    if traces is not None:
        res["kernel_trace"] = traces
        ds = next((v for k, v in traces.items() if "depth_sensor_kernel" in k), None)
        op = next((v for k, v in traces.items() if "obs_post_kernel" in k), None)
        if ds and op:
            res["kernel_time_ratio"] = ds["average_us"] / op["average_us"]
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
