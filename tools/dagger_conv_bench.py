#!/usr/bin/env python3
"""Times the fused DAgger path of the 160 x 90 student (isaac_rover_orbit_amd.dagger_conv) on the GPU, beside the 31 x 31 student's
update and the torch specification in the same run.

    python tools/dagger_conv_bench.py [--reps 7] [--steps 30] [--out profiles/dagger_conv_bench.json] [--no-env] [--trace]

Items, alternated in one process; per item a host clock around --steps back-to-back calls that ends in a device synchronise, divided by
--steps; median, min and max over --reps rounds after a warm-up (tools/dagger_bench.py's method):

  conv_update          one FusedConvDAgger.update at --batch rows of a --slots x --envs memory and image ring of seeded synthetic data
  dagger_update        one FusedDAgger.update (the 31 x 31 student: no stem, no images) at the same batch on the same memory
  torch_conv_update    TorchConvDAgger in float32 on the same device (with its gathers), for scale
  render_160x90        RoverEnv.render_depth() of --envs envs at the default camera (reported, not targeted)
  collect              ConvDAggerCollector.record + act on --envs envs: x into the image ring, stem, rows, teacher, student, mix, indices
  collector_step       render_160x90 + collect

--trace: before this process opens the GPU, a child process runs the update items alone under ``rocprofv3 --kernel-trace --stats``;
the average device time of the stem's forward and backward kernels, and the bytes per second over the --batch x 57.6 KB of images each
reads, go into the result under "stem_kernels" (null with the reason when the profiler is not there).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

IMAGE_BYTES = 4 * 14400
NOT_MEASURED = ["learning curves", "multi-GPU", "batches other than --batch", "the torch collector on the device"]


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def summary(xs):
    return {"median_ms": 1e3 * statistics.median(xs), "min_ms": 1e3 * min(xs), "max_ms": 1e3 * max(xs), "n": len(xs)}


def trace_stem_kernels(args):
    """Average device time of the stem's kernels from a child run of the update items under the kernel trace."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return {"skipped": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--no-env", "--reps", "1",
               "--steps", "10", "--envs", str(args.envs), "--slots", str(args.slots), "--batch", str(args.batch)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            return {"skipped": f"the traced child ended with {r.returncode}"}
        rows = []
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        for path in found:
            with open(path, newline="") as f:
                rows += list(csv.DictReader(f))
        if not rows:
            return {"skipped": "no kernel_stats.csv among " + ", ".join(sorted(os.path.basename(p) for p in
                                                                              glob.glob(os.path.join(tmp, "**", "*"), recursive=True))[:12])}
    out = {}
    for r in rows:
        name = r.get("Name", "")
        for key in ("dagger_conv_forward_kernel", "dagger_conv_backward_kernel", "rover_dagger_conv_rows_kernel"):
            if key in name:
                ns = float(r["AverageNs"])
                out[key] = {"calls": int(r["Calls"]), "average_us": ns / 1e3,
                            "image_bytes": args.batch * IMAGE_BYTES if "rows" not in key else None,
                            "image_GB_per_s": args.batch * IMAGE_BYTES / ns if "rows" not in key else None}
    return out or {"skipped": "no stem kernel in the trace"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--no-env", action="store_true", help="the update items only")
    ap.add_argument("--trace", action="store_true", help="also the stem kernels' device times from a traced child process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stem_kernels = trace_stem_kernels(args) if args.trace else None      # before this process opens the GPU
    import torch
    from ppo_reference import load_example
    from isaac_rover_orbit_amd import dagger, dagger_conv
    from isaac_rover_orbit_amd.policy import RoverNet
    from isaac_rover_orbit_amd.td3 import ReplayMemory
    ex = load_example()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    student, teacher = ex.Net(2, True).to(dev), ex.Net(2, True).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    mem, ring = ReplayMemory(args.slots, args.envs, device=dev), dagger_conv.ImageRing(args.slots, args.envs, dev)
    mem.obs.copy_(torch.randn(mem.obs.shape, device=dev, generator=g) * 0.5)
    mem.actions.copy_(torch.rand(mem.actions.shape, device=dev, generator=g) * 2 - 1)
    mem.ring_pos.copy_(torch.arange(args.slots, dtype=torch.int32, device=dev))
    mem.filled, mem.memory_index, mem.cursor = True, 0, args.slots
    ring.x.copy_(torch.rand(ring.x.shape, device=dev, generator=g))
    B = args.batch
    idx = mem.sample_indices(B, g)
    conv = dagger_conv.FusedConvDAgger(student.state_dict(), seed=0)
    fused = dagger.FusedDAgger(student.state_dict())
    spec = dagger_conv.TorchConvDAgger(ex.Net(2, True).to(dev), dagger_conv.ConvStem.seeded(0).to(dev))
    items = [("conv_update", lambda: conv.update(mem, ring, idx)), ("dagger_update", lambda: fused.update(mem, idx))]
    torch_note = None
    try:                                        # torch's convolution of this shape on the device is the library's to provide
        spec.update(mem, ring, idx)
        torch.cuda.synchronize()
        items.append(("torch_conv_update", lambda: spec.update(mem, ring, idx)))
    except RuntimeError as e:
        torch_note = f"not measured: {str(e).splitlines()[0][:200]}"
    env = None
    if not args.no_env:
        from isaac_rover_orbit_amd import terrain as T
        from isaac_rover_orbit_amd.cfg import RoverEnvCfg
        from isaac_rover_orbit_amd.envs import RoverEnv
        terrain = T.make_procedural_terrain((2048, 2048), seed=1234)
        terrain.make_spawns(2 * args.envs)
        cfg = RoverEnvCfg(); cfg.scene.num_envs = args.envs; cfg.terrain.kind = "custom"; cfg.camera = dagger_conv.student_camera_cfg()
        env = RoverEnv(cfg, terrain=terrain)
        obs, _ = env.reset()
        obs, rew, term, _, _ = env.step(torch.zeros(args.envs, 2, device=dev))
        rows, depth = obs["policy"].clone(), env.render_depth()
        cmem, cring = ReplayMemory(args.slots, args.envs, device=dev), dagger_conv.ImageRing(args.slots, args.envs, dev)
        col = dagger_conv.ConvDAggerCollector(RoverNet.from_state_dict(teacher.state_dict(), final_act="tanh"), conv, cmem, cring)
        col.begin(rows, depth)

        def collect():
            col.act(0.5)
            col.record(rows, depth, rew, term, B)

        def collector_step():
            d = env.render_depth()
            col.act(0.5)
            col.record(rows, d, rew, term, B)

        items += [("render_160x90", env.render_depth), ("collect", collect), ("collector_step", collector_step)]
    res = {k: [] for k, _ in items}
    for _ in range(3):                          # warm-up
        for _, fn in items:
            fn()
    for _ in range(args.reps):
        for k, fn in items:
            res[k].append(timed(fn, args.steps))
    st = conv.stats()
    out = {"rows": B, "memory_slots": args.slots, "envs": args.envs, "reps": args.reps, "steps": args.steps,
           "device": torch.cuda.get_device_name(0), **{k: summary(v) for k, v in res.items()},
           "conv_over_dagger_update": statistics.median(res["conv_update"]) / statistics.median(res["dagger_update"]),
           "conv_over_torch_update": (statistics.median(res["conv_update"]) / statistics.median(res["torch_conv_update"])
                                      if "torch_conv_update" in res else torch_note),
           "image_bytes_per_pass": B * IMAGE_BYTES, "stem_kernels": stem_kernels,
           "conv_stats": {k: st[k] for k in ("steps", "bad_index", "loss", "grad_norm")}, "not_measured": NOT_MEASURED}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if env is not None:
        env.close()


if __name__ == "__main__":
    main()
