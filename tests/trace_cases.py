"""Shared by test_trace_collect.py and test_gpu_trace_collect.py: drive ``trace.EpisodeRecorder`` (the specification) and a
collector under test with identical per-step tensors from a seeded generator, and compare the files bit for bit."""
import os

import numpy as np
import torch

from isaac_rover_orbit_amd.trace import EpisodeRecorder, load_trace

EXTRAS = {"feat": {"shape": (5, 2), "dtype": np.float32}, "tag": {"shape": (3,), "dtype": np.uint8}}
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8}


def step_tensors(g, n, obs_dim, act_dim, extras, special=False):
    """One step's tensors on the CPU.  ``special``: NaNs with payloads, -0.0 and both infinities in observations and rewards."""
    obs, act, rew = torch.randn(n, obs_dim, generator=g), torch.randn(n, act_dim, generator=g), torch.randn(n, generator=g)
    if special:
        bits = torch.tensor([0x7FC00001, 0xFFC12345 - (1 << 32), 0x7F800001, -(1 << 31), 0x7F800000, 0xFF800000 - (1 << 32)], dtype=torch.int32)
        vals = bits.view(torch.float32)                                  # quiet / signalling NaNs with payloads, -0.0, +inf, -inf
        pos = torch.randint(0, obs_dim, (n, vals.numel()), generator=g)
        obs[torch.arange(n)[:, None], pos] = vals[None, :].expand(n, -1)
        rew.view(torch.int32)[:] = bits[torch.randint(0, bits.numel(), (n,), generator=g)]
    info = {}
    for k, p in (extras or {}).items():
        dt = _TORCH[np.dtype(p["dtype"])]
        shape = (n, *p["shape"])
        info[k] = torch.randint(0, 256, shape, generator=g).to(torch.uint8) if dt == torch.uint8 else torch.randn(shape, generator=g)
    return obs, act, rew, info


def drive(make, tmp, n, steps, p_done, max_ep, obs_dim=7, act_dim=2, extras=EXTRAS, max_rows=40, seed=0, device="cpu", special=False,
          done_fn=None, force=True, hook=None, to_device=None, close=True):
    """Runs the specification and ``make(base_filename)`` side by side.  ``done_fn(t, n) -> bool tensor`` overrides the Bernoulli
    done flags; with ``force`` an env is done when its episode reaches ``max_ep`` rows (its time-out).  ``hook(col, t)`` runs after
    step t's append.  ``to_device(name, tensor)`` places a tensor on the device (default: ``.to(device)``).  Returns
    (spec recorder, collector, spec files, collector files)."""
    os.makedirs(os.path.join(tmp, "ref"), exist_ok=True)
    os.makedirs(os.path.join(tmp, "dev"), exist_ok=True)
    ref = EpisodeRecorder(os.path.join(tmp, "ref", "run"), n, obs_dim, act_dim, extras, max_rows=max_rows)
    col = make(os.path.join(tmp, "dev", "run"))
    g = torch.Generator().manual_seed(1234 + seed)
    length = torch.zeros(n, dtype=torch.int64)
    put = to_device or (lambda name, x: x.to(device))
    for t in range(steps):
        obs, act, rew, info = step_tensors(g, n, obs_dim, act_dim, extras, special)
        done = done_fn(t, n) if done_fn is not None else torch.rand(n, generator=g) < p_done
        length += 1
        if force:
            done = done | (length >= max_ep)
        length[done] = 0
        ref.append_to_buffer(obs, act, rew, done, info)
        col.append(put("obs", obs), put("act", act), put("rew", rew), put("done", done), {k: put(k, v) for k, v in info.items()})
        if hook is not None:
            hook(col, t)
    if not close:
        return ref, col, None, None
    return ref, col, ref.close(), col.close()


def assert_same_files(ref_files, got_files):
    """File count and names, number_of_steps, dtype and shape of every dataset, and the dataset BYTES (NaN payloads count)."""
    assert [os.path.basename(f) for f in got_files] == [os.path.basename(f) for f in ref_files]
    for fr, fg in zip(ref_files, got_files):
        a, b = load_trace(fr), load_trace(fg)
        assert sorted(a) == sorted(b), (fr, sorted(a), sorted(b))
        assert a["number_of_steps"] == b["number_of_steps"], (fr, a["number_of_steps"], b["number_of_steps"])
        for k in a:
            if k == "number_of_steps":
                continue
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (fr, k, a[k].dtype, b[k].dtype, a[k].shape, b[k].shape)
            assert np.array_equal(np.ascontiguousarray(a[k]).reshape(-1).view(np.uint8),
                                  np.ascontiguousarray(b[k]).reshape(-1).view(np.uint8)), (fr, k)
    return [load_trace(f)["number_of_steps"] for f in ref_files]
