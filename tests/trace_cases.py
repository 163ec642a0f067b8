"""Shared by test_trace_collect.py and test_gpu_trace_collect.py: drive ``trace.EpisodeRecorder`` (the specification) and a
collector under test with identical per-step tensors from a seeded generator, and compare the files bit for bit."""
import os

import numpy as np
import torch

from isaac_rover_orbit_amd.trace import EpisodeRecorder, load_trace

EXTRAS = {"feat": {"shape": (5, 2), "dtype": np.float32}, "tag": {"shape": (3,), "dtype": np.uint8}}
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.float64): torch.float64,
          np.dtype(np.float16): torch.float16, np.dtype(np.int8): torch.int8, np.dtype(np.int16): torch.int16,
          np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.bool_): torch.bool}
_INT_RANGE = {torch.int8: (-128, 128), torch.int16: (-2 ** 15, 2 ** 15), torch.int32: (-2 ** 31, 2 ** 31), torch.int64: (-2 ** 62, 2 ** 62)}


def _extra_tensor(g, dt, shape):
    """Random rows of every dtype trace_collect._TORCH_OF accepts; float32 and uint8 draw what they always drew."""
    if dt == torch.uint8:
        return torch.randint(0, 256, shape, generator=g).to(torch.uint8)
    if dt == torch.float32:
        return torch.randn(shape, generator=g)
    if dt == torch.bool:
        return torch.randint(0, 2, shape, generator=g).to(torch.bool)
    if dt in _INT_RANGE:
        return torch.randint(*_INT_RANGE[dt], shape, generator=g).to(dt)
    return torch.randn(shape, generator=g, dtype=torch.float64).to(dt)           # float64, float16


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
        info[k] = _extra_tensor(g, _TORCH[np.dtype(p["dtype"])], (n, *p["shape"]))
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


# ---------------------------------------------------------------------------------------------- edges (test_*trace_collect*)
def _u8(k):
    return {"shape": (k,), "dtype": np.uint8}


# row widths around the narrow / wide boundary (16 bytes) ...
NARROW_EDGE = {"u16": _u8(16), "u17": _u8(17), "i16x9": {"shape": (9,), "dtype": np.int16}, "f32x5": {"shape": (5,), "dtype": np.float32},
               "f64x3": {"shape": (3,), "dtype": np.float64}, "i64x1": {"shape": (1,), "dtype": np.int64}}
# ... and around one span / two spans (4096 bytes), with tails of 0, 1, 2 and 4 bytes behind the last 16-byte piece
SPAN_EDGE = {"u4096": _u8(4096), "u4097": _u8(4097), "f32x1025": {"shape": (1025,), "dtype": np.float32},
             "f16x2049": {"shape": (2049,), "dtype": np.float16}}
# exactly 12 extras: with the four fixed datasets that is ROVER_TRACE_MAX_STREAMS
SIXTEEN_STREAMS = dict(NARROW_EDGE, **SPAN_EDGE, **EXTRAS)
assert len(SIXTEEN_STREAMS) == 12
WIDTH_CASES = {"narrow_edge": NARROW_EDGE, "span_edge": SPAN_EDGE, "sixteen_streams": SIXTEEN_STREAMS}
WIDTH_STEPS = {5: 24, 67: 12}                      # by env count: rings of 9 rows wrap twice / once (the files are 16 KB a row)

# done patterns of the commit-carry cases (n > 512: three chunks of 256 envs): t, n -> bool (n,)
CARRY_PATTERNS = {"env_0": lambda t, n: torch.arange(n) == 0,
                  "envs_255_256": lambda t, n: (torch.arange(n) == 255) | (torch.arange(n) == 256),
                  "envs_63_64_511_512": lambda t, n: torch.isin(torch.arange(n), torch.tensor([63, 64, 511, 512])),
                  "every_env": lambda t, n: torch.ones(n, dtype=torch.bool),
                  "odd_envs": lambda t, n: torch.arange(n) % 2 == 1}
CARRY_KW = dict(max_episode_rows=8, drain_interval=3, piece_rows=64)
NEVER = 1 << 30                                    # a drain interval no test reaches


def pitched_sources(n, obs_dim, device="cpu", seed=7):
    """A ``to_device`` for ``drive``: the observation as ``big[:, 3:3 + obs_dim]`` of an (n, obs_dim + 40) tensor, the reward as an
    (n, 3) tensor whose first column counts, the extra "feat" as the row slice ``big[1:n + 1]``; everything around the recorded
    values is noise, so a wrong pitch or offset shows in the files."""
    g = torch.Generator().manual_seed(seed)

    def put(name, x):
        if name == "obs":
            big = torch.randn(n, obs_dim + 40, generator=g).to(device)
            view = big[:, 3:3 + obs_dim]
        elif name == "rew":
            big = torch.randn(n, 3, generator=g).to(device)
            view = big[:, 0]
            view.copy_(x)
            return big
        elif name == "feat":
            big = torch.randn(n + 2, *x.shape[1:], generator=g).to(device)
            view = big[1:n + 1]
        else:
            return x.to(device)
        view.copy_(x)
        return view
    return put


def uint8_done(device="cpu"):
    """A ``to_device`` for ``drive``: done flags as uint8 holding 1, 2 and 255 (in turn over envs and steps) where the flag is set."""
    calls = [0]

    def put(name, x):
        if name != "done":
            return x.to(device)
        calls[0] += 1
        vals = torch.tensor([1, 2, 255], dtype=torch.uint8)[(torch.arange(x.numel()) + calls[0]) % 3]
        return torch.where(x, vals, torch.zeros_like(vals)).to(device)
    return put


def state_words(col):
    """The collector's state block on the host as int32 (synchronises)."""
    return col.state.cpu().numpy().copy()


def assert_same_state(col, model):
    """The state block of a ``TraceCollector`` word for word against a ``TorchTraceCollector`` driven by the same calls: header
    words 0 .. 2 (count, status, rows), head[n], len[n], pending[n] and the first min(count, desc_cap) descriptors."""
    from isaac_rover_orbit_amd import trace_collect as TC
    assert (col.n, col.R, col.desc_cap) == (model.n, model.R, model.desc_cap)
    a, b = state_words(col), state_words(model)
    n, H = col.n, TC.HEADER_WORDS
    assert a[:3].tolist() == b[:3].tolist(), ("count, status, rows", a[:3].tolist(), b[:3].tolist())
    for j, name in enumerate(("head", "len", "pending")):
        x, y = a[H + j * n:H + (j + 1) * n], b[H + j * n:H + (j + 1) * n]
        assert np.array_equal(x, y), (name, np.flatnonzero(x != y)[:8].tolist())
    k, d0 = min(int(a[TC.W_COUNT]), col.desc_cap), TC.desc_word(n)
    x, y = a[d0:d0 + 4 * k].reshape(k, 4), b[d0:d0 + 4 * k].reshape(k, 4)
    assert np.array_equal(x, y), ("descriptors", np.flatnonzero((x != y).any(1))[:8].tolist())


def model_base(base):
    """The base file name of a model that runs beside the collector of ``base``: the same name in a directory of its own."""
    d = os.path.dirname(base) + "_model"
    os.makedirs(d, exist_ok=True)
    return os.path.join(d, os.path.basename(base))


class Paired:
    """A collector and its CPU model behind one ``append`` / ``drain`` / ``close``: both get the same calls, the model's own drains
    are held back, and in front of every drain of the collector (those ``append`` and ``close`` start included) the two state
    blocks are compared and the model drains first.  ``checks`` counts the comparisons."""

    def __init__(self, col, model):
        self.col, self.model, self.checks, self.model_files = col, model, 0, None
        model.interval = NEVER
        inner = col.drain

        def drain():
            assert_same_state(col, model)
            self.checks += 1
            model.drain()
            return inner()
        col.drain = drain

    def append(self, obs, act, rew, done, info=None):
        self.model.append(obs.cpu(), act.cpu(), rew.cpu(), done.cpu(), None if info is None else {k: v.cpu() for k, v in info.items()})
        self.col.append(obs, act, rew, done, info)

    def drain(self):
        self.col.drain()

    def close(self):
        if not self.model._closed:
            self.model._commit_all()                 # what col.close() does in front of its drain
        files = self.col.close()
        self.model_files = self.model.close()
        return files


# ring and descriptor overrun: max_episode_rows = 6 and drain_interval = 3 give R = 9 and desc_cap = 4 n; the drain is held off.
#   desc: every env done at every step, 8 one-row episodes per env: step t commits descriptors [t n, (t + 1) n), so the list of 4 n
#         is first overrun at step 4, and 8 pending rows never fill the ring of 9
#   ring: every env done at every third step: three 3-row episodes fill the ring at step 8 (3 n descriptors <= 4 n), and the row of
#         step 9 is the first one refused
OVERRUN_KW = dict(max_episode_rows=6, drain_interval=3, guard_bytes=64)
OVERRUN = {"desc": dict(done=lambda t: True, steps=8, first=4, bit=4, match="descriptor list"),
           "ring": dict(done=lambda t: t % 3 == 2, steps=12, first=9, bit=2, match="ring")}


def drive_overrun(collectors, kind, n, after_step=None, obs_dim=7, extras=EXTRAS):
    """The same steps into every collector of ``collectors`` (each on its own device) with the drain held off."""
    case, g = OVERRUN[kind], torch.Generator().manual_seed(77)
    for c in collectors:
        assert (c.R, c.desc_cap) == (9, 4 * n)
        c.interval = NEVER
    for t in range(case["steps"]):
        obs, act, rew, info = step_tensors(g, n, obs_dim, 2, extras)
        done = torch.full((n,), bool(case["done"](t)))
        for c in collectors:
            c.append(obs.to(c.device), act.to(c.device), rew.to(c.device), done.to(c.device), {k: v.to(c.device) for k, v in info.items()})
        if after_step is not None:
            after_step(t, 0 if t < case["first"] else case["bit"])
