"""Episode traces recorded on the device: fused append, commit and gather (include/rover_trace.h).

``trace.EpisodeRecorder`` is the specification of the files: per env step one row of every dataset joins its env's open episode,
and a done env's episode goes to the current file as one contiguous block, in (step of completion, env id) order.  It does so on
the host: a synchronising copy of every tensor per step and a Python loop over the envs.  ``TraceCollector`` writes the SAME files
(bit for bit, for the same sequence of calls) and keeps the rows on the device in between::

    col = TraceCollector("traces/run", env.num_envs, 965, 2, env=env)          # max_episode_rows = env.max_episode_length
    loop:
        obs, rew, terminated, truncated, info = env.step(actions)
        col.append(last_obs, actions, rew, terminated | truncated)               # two launches, nothing read back
    files = col.close()

Per step ``append`` issues one ``rover_trace_append``: a launch that stages every stream's rows into per-env rings of
``R = max_episode_rows + drain_interval`` rows, and a single-workgroup launch that commits the finished episodes, in env-id order, to
a device list of ``(env, start, len, offset)`` descriptors.  Every ``drain_interval`` steps (and on ``drain()`` / ``close()``) the
collector synchronises once, reads the counters and the list, gathers the committed episodes ``piece_rows`` output rows at a time
into packed blocks, copies each block to the host and hands whole episodes to ``EpisodeRecorder``'s own writer, which decides
the file roll-over as it always did.

Why the ring never overflows: between two drains an env's ring holds the rows of its unfinished episode at the last drain (at most
``max_episode_rows``) plus the rows staged since (at most ``drain_interval``), and everything committed before the last drain is
free again.  An episode that outgrows ``max_episode_rows`` is not staged (so nothing is overwritten); a sticky status word records
it and the next drain raises ``TraceOverflowError``.

The tensors must be what the files hold: float32 observations / actions / rewards, bool (or uint8) done flags, extras of their
declared dtype.  A source tensor needs no particular alignment; each env's elements must form one dense block (any permutation of
a contiguous block, e.g. ``extras["depth"]``'s ``permute(0, 2, 1)`` view: the block is recorded as it lies and the permutation is
re-applied on the host at the drain).

``TorchTraceCollector`` is the same ring / descriptor / piecewise-gather scheme in plain torch on the CPU: the model of the kernels.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _fused, _lib
from .trace import EpisodeRecorder

HEADER_WORDS = 16                 # include/rover_trace.h
W_COUNT, W_STATUS, W_ROWS = 0, 1, 2
COMMIT_CHUNK = 256                # envs the commit kernel visits per pass
MAX_STREAMS = 16
FLAG_BOOL = 1
ST_EPISODE, ST_RING, ST_DESC = 1, 2, 4
DEFAULT_PIECE_BYTES = 64 << 20    # default piece_rows: as many output rows as fit 64 MiB over all streams


class TraceOverflowError(RuntimeError):
    """An episode outgrew ``max_episode_rows`` (or the ring / the descriptor list was overrun): raised by the next drain."""


def stage_pitch(row_bytes: int) -> int:
    """Bytes between two staged rows: ``row_bytes`` rounded up to 16 (rows of 16 bytes or more) or to 4 (rover_trace_stage_pitch)."""
    a = 16 if row_bytes >= 16 else 4
    return (int(row_bytes) + a - 1) // a * a


def desc_word(n: int) -> int:
    """Word of the state block at which the descriptors start (16-byte aligned behind head[n], len[n], pending[n])."""
    return HEADER_WORDS + ((3 * int(n) + 3) & ~3)


def state_bytes(n: int, desc_cap: int) -> int:
    return 4 * (desc_word(n) + 4 * int(desc_cap))


def _stream_specs(obs_dim: int, act_dim: int, extras: dict | None):
    """[(dataset, row shape, numpy dtype, row bytes, flags)] in ``EpisodeRecorder.keys`` order."""
    specs = [("observations", (int(obs_dim),), np.dtype(np.float32), 0), ("actions", (int(act_dim),), np.dtype(np.float32), 0),
             ("rewards", (1,), np.dtype(np.float32), 0), ("terminated", (1,), np.dtype(np.bool_), FLAG_BOOL)]
    for k, p in (extras or {}).items():
        specs.append((k, tuple(int(x) for x in p["shape"]), np.dtype(p["dtype"]), 0))
    out = []
    for k, shape, dt, flags in specs:
        rb = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        if rb <= 0:
            raise ValueError(f"dataset {k!r} has empty rows")
        out.append((k, shape, dt, rb, flags))
    if len(out) > MAX_STREAMS:
        raise ValueError(f"at most {MAX_STREAMS} datasets (4 + {MAX_STREAMS - 4} extras)")
    return out


_TORCH_OF = {np.dtype(np.float32): (torch.float32,), np.dtype(np.float64): (torch.float64,), np.dtype(np.float16): (torch.float16,),
             np.dtype(np.uint8): (torch.uint8,), np.dtype(np.int8): (torch.int8,), np.dtype(np.int16): (torch.int16,),
             np.dtype(np.int32): (torch.int32,), np.dtype(np.int64): (torch.int64,), np.dtype(np.bool_): (torch.bool, torch.uint8)}


class _TraceBase:
    """Arguments, layout, buffers, the drain's host side and the writer: everything but the four device operations."""

    def __init__(self, base_filename: str, num_envs: int, obs_dim: int, act_dim: int, extras: dict | None = None,
                 max_rows: int = 500_000, backend: str = "auto", max_episode_rows: int | None = None, drain_interval: int = 64,
                 piece_rows: int | None = None, device=None, env=None, guard_bytes: int = 0):
        # the writer IS EpisodeRecorder (one slot: whole episodes are handed to its write_to_disk); it validates base_filename / backend
        self.writer = EpisodeRecorder(base_filename, 1, obs_dim, act_dim, extras, max_rows, backend)
        if max_episode_rows is None:
            if env is None or not hasattr(env, "max_episode_length"):
                raise ValueError("give max_episode_rows, or env= (an env or a cfg with max_episode_length)")
            max_episode_rows = int(env.max_episode_length)
        self.n, self.max_ep, self.interval = int(num_envs), int(max_episode_rows), int(drain_interval)
        if self.n < 1 or self.max_ep < 1 or self.interval < 1:
            raise ValueError("num_envs, max_episode_rows and drain_interval must be >= 1")
        self.specs = _stream_specs(obs_dim, act_dim, extras)
        self.keys = [s[0] for s in self.specs]
        self.R = self.max_ep + self.interval
        self.desc_cap = self.n * (self.interval + 1)
        if self.n * self.R >= 2 ** 31:
            raise ValueError("num_envs * (max_episode_rows + drain_interval) must stay below 2**31")
        self.piece = self.default_piece_rows(self.n, obs_dim, act_dim, extras, self.max_ep, self.interval) if piece_rows is None else int(piece_rows)
        if self.piece < 1:
            raise ValueError("piece_rows must be >= 1")
        self.device = torch.device(device)
        self._guard = int(guard_bytes)
        self._raw = []                                       # every allocation, guard included
        self.state = self._alloc(state_bytes(self.n, self.desc_cap)).view(torch.int32)
        self.stage = [self._alloc(self.n * self.R * stage_pitch(rb)) for _, _, _, rb, _ in self.specs]
        self.out = [self._alloc(self.piece * rb) for _, _, _, rb, _ in self.specs]
        self._perm = [None] * len(self.specs)                # per stream: how an env's block is permuted back on the host
        self._steps, self._since, self._failed, self._closed = 0, 0, False, False
        self.calls: list = []                                # (C entry point, kernel launches) of every device call, in order

    # ------------------------------------------------------------------------------------------------------------- sizes
    @staticmethod
    def default_piece_rows(num_envs, obs_dim, act_dim, extras=None, max_episode_rows=750, drain_interval=64) -> int:
        row = sum(s[3] for s in _stream_specs(obs_dim, act_dim, extras))
        return max(1, min(int(num_envs) * (int(max_episode_rows) + int(drain_interval)), DEFAULT_PIECE_BYTES // row))

    @staticmethod
    def device_bytes(num_envs, obs_dim, act_dim, extras=None, max_episode_rows=750, drain_interval=64, piece_rows=None) -> int:
        """Bytes the collector allocates on its device: state block + rings + output blocks.  The rings dominate:
        ``num_envs * (max_episode_rows + drain_interval) * sum(stage_pitch(row_bytes))``, e.g. 3.9 KB per env step without extras and
        61.5 KB with the depth image (57.6 KB)."""
        n, R = int(num_envs), int(max_episode_rows) + int(drain_interval)
        specs = _stream_specs(obs_dim, act_dim, extras)
        if piece_rows is None:
            piece_rows = _TraceBase.default_piece_rows(n, obs_dim, act_dim, extras, max_episode_rows, drain_interval)
        return (state_bytes(n, n * (int(drain_interval) + 1)) + sum(n * R * stage_pitch(s[3]) for s in specs)
                + sum(int(piece_rows) * s[3] for s in specs))

    def _alloc(self, nbytes: int) -> torch.Tensor:
        raw = torch.zeros(nbytes + self._guard, dtype=torch.uint8, device=self.device)
        if self._guard:
            raw[nbytes:] = 0xA5
        self._raw.append((raw, nbytes))
        return raw[:nbytes]

    def allocated_bytes(self) -> int:
        return sum(nbytes for _, nbytes in self._raw)

    def guards_intact(self) -> bool:
        """With ``guard_bytes > 0`` every buffer is followed by that many canary bytes; true while none of them changed."""
        return all(bool((raw[nbytes:] == 0xA5).all()) for raw, nbytes in self._raw)

    # ----------------------------------------------------------------------------------------------------------- sources
    def _dense(self, i: int, t: torch.Tensor, lead: int | None = None):
        """(tensor keeping the memory alive, element offset 0 view) -> (t2, pitch_bytes): ``t2[e]`` starts env e's dense block.  For a
        permuted view the permutation back is remembered in ``self._perm[i]``."""
        key, shape, dt, rb, _ = self.specs[i]
        if not isinstance(t, torch.Tensor) or t.dtype not in _TORCH_OF[dt][:2 if i == 3 else 1] or t.device != self.device:
            raise ValueError(f"{key} must be a {_TORCH_OF[dt][0]} tensor on {self.device}")
        if t.dim() == 0 or t.shape[0] != self.n:
            raise ValueError(f"{key} must have {self.n} rows")
        if t.dim() == 1:
            t = t.unsqueeze(1)
        elems = rb // dt.itemsize
        per_env = t[0].numel()
        if lead is None and (per_env != elems or (len(shape) > 1 and tuple(t.shape[1:]) != shape)):
            raise ValueError(f"{key} must have shape ({self.n}, {', '.join(map(str, shape))})")
        if lead is not None and per_env < lead:
            raise ValueError(f"{key} must have at least {lead} column(s)")
        order = sorted(range(1, t.dim()), key=lambda d: (-t.stride(d), d))
        tp = t.permute(0, *order)
        want = 1
        for d in range(tp.dim() - 1, 0, -1):
            if tp.shape[d] != 1 and tp.stride(d) != want:
                raise ValueError(f"{key}: each env's elements must form one dense block (a permuted contiguous tensor is fine)")
            want *= tp.shape[d]
        if self.n > 1 and tp.stride(0) < want:
            raise ValueError(f"{key}: rows overlap")
        perm = None
        if order != list(range(1, t.dim())) and lead is None:
            inv = [0] * len(order)
            for pos, d in enumerate(order):
                inv[d - 1] = pos
            perm = (tuple(tp.shape[1:]), tuple(inv))
        if self._steps and self._perm[i] != perm:
            raise ValueError(f"{key}: the memory layout must not change between steps")
        self._perm[i] = perm
        return tp, (tp.stride(0) if self.n > 1 else want) * dt.itemsize

    def append(self, obs, action, reward, done, info=None) -> None:
        """One env step of every env.  ``done``: bool / uint8, one flag per env.  ``info``: the dict holding the extras."""
        if self._closed or self._failed:
            raise RuntimeError("the collector is closed" if self._closed else "the collector failed earlier")
        if isinstance(obs, dict):
            obs = obs["policy"]
        src = [self._dense(0, obs), self._dense(1, action), self._dense(2, reward, lead=1), self._dense(3, done, lead=1)]
        if done.numel() != self.n or not done.is_contiguous():
            raise ValueError(f"done must hold one contiguous flag per env ({self.n})")
        for i in range(4, len(self.specs)):
            if info is None or self.keys[i] not in info:
                raise ValueError(f"info lacks the extra {self.keys[i]!r}")
            src.append(self._dense(i, info[self.keys[i]]))
        self._append(src, done)
        self._steps += 1
        self._since += 1
        if self._since >= self.interval:
            self.drain()

    # ------------------------------------------------------------------------------------------------------------- drain
    def _rows_of(self, i: int, block: np.ndarray) -> np.ndarray:
        """(m * row_bytes,) uint8 -> (m, *shape) of the dataset's dtype, the recorded permutation undone."""
        _, shape, dt, rb, _ = self.specs[i]
        a = block.view(dt).reshape(-1, *(self._perm[i][0] if self._perm[i] else shape))
        if self._perm[i]:
            a = np.ascontiguousarray(a.transpose(0, *(1 + p for p in self._perm[i][1])))
        return a

    def _emit(self, parts: list) -> None:
        w = self.writer
        w.buffers[0] = {k: (parts[0][k] if len(parts) == 1 else np.concatenate([p[k] for p in parts], 0)) for k in w.keys}
        w.write_to_disk(0)

    def drain(self) -> None:
        """Synchronise once, write every committed episode to the files, empty the descriptor list."""
        if self._closed:
            raise RuntimeError("the collector is closed")
        if self._failed:
            raise RuntimeError("the collector failed earlier")
        self._since = 0
        count, status, rows, desc = self._read_state()
        if status:
            self._failed = True
            what = [w for b, w in ((ST_EPISODE, f"an episode outgrew max_episode_rows = {self.max_ep}"), (ST_RING, "a ring was overrun"),
                                   (ST_DESC, "the descriptor list was overrun")) if status & b]
            raise TraceOverflowError("; ".join(what) + " (status %d); nothing of this drain was written" % status)
        if count == 0:
            return
        try:
            pos, parts = 0, []
            for r0 in range(0, rows, self.piece):
                m = min(self.piece, rows - r0)
                blocks = self._gather(r0, m)
                data = {k: self._rows_of(i, blocks[i]) for i, k in enumerate(self.keys)}
                while pos < count and int(desc[pos, 3]) < r0 + m:
                    off, ln = int(desc[pos, 3]), int(desc[pos, 2])
                    a, b = max(off, r0) - r0, min(off + ln, r0 + m) - r0
                    parts.append({k: v[a:b] for k, v in data.items()})
                    if off + ln > r0 + m:
                        break                                # the episode goes on in the next piece
                    self._emit(parts)
                    pos, parts = pos + 1, []
        except Exception:
            self._failed = True
            raise
        self._drained()

    def close(self) -> list:
        """Commit every open non-empty episode in env-id order, drain, close the file; returns the file names."""
        if self._closed:
            return list(self.writer.files)
        try:
            if not self._failed:
                self._commit_all()
                self.drain()
        finally:
            self._closed = True
            self.writer.buffers[0] = self.writer._empty()
            self.writer.close()
        return list(self.writer.files)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ------------------------------------------------------------------------------------------------------------------ the model
class TorchTraceCollector(_TraceBase):
    """The ring / descriptor / piecewise-gather scheme in plain torch on the CPU, on the same buffers with the same layout."""

    def __init__(self, *args, device="cpu", **kw):
        super().__init__(*args, device=device, **kw)

    def _views(self):
        n = self.n
        s = self.state
        return s[HEADER_WORDS:HEADER_WORDS + n], s[HEADER_WORDS + n:HEADER_WORDS + 2 * n], s[HEADER_WORDS + 2 * n:HEADER_WORDS + 3 * n], \
            s[desc_word(n):].view(self.desc_cap, 4)

    def _append(self, src, done) -> None:
        head, ln, pend, desc = self._views()
        ok = (ln < self.max_ep) & (pend + ln < self.R)
        ids = ok.nonzero().flatten()
        slot = ((head + ln) % self.R).long()[ids]
        for i, (t, _) in enumerate(src):
            _, _, dt, rb, flags = self.specs[i]
            rows = t.reshape(self.n, -1)[:, :rb // dt.itemsize].contiguous()
            rows = (rows != 0).to(torch.uint8) if flags & FLAG_BOOL else rows.view(torch.uint8)
            self.stage[i].view(self.n, self.R, stage_pitch(rb))[ids, slot, :rb] = rows[ids]
        self._commit(done.reshape(self.n) != 0, False)

    def _commit(self, done, everything: bool) -> None:
        head, ln, pend, desc = self._views()
        s = self.state
        if not everything:
            ep = ln >= self.max_ep
            ring = ~ep & (pend + ln >= self.R)
            ln += (~ep & ~ring).to(torch.int32)
            s[W_STATUS] |= ST_EPISODE * int(ep.any()) | ST_RING * int(ring.any())
        emit = (ln > 0) if everything else (done & (ln > 0))
        ids = emit.nonzero().flatten()                       # ascending env id
        if ids.numel() == 0:
            return
        ls = ln[ids]
        offs = int(s[W_ROWS]) + torch.cumsum(ls, 0, dtype=torch.int32) - ls
        idx = int(s[W_COUNT]) + torch.arange(ids.numel())
        fits = idx < self.desc_cap
        desc[idx[fits]] = torch.stack([ids.to(torch.int32), head[ids], ls, offs], 1)[fits]
        if not bool(fits.all()):
            s[W_STATUS] |= ST_DESC
        head[ids] = (head[ids] + ls) % self.R
        pend[ids] += ls
        s[W_COUNT] += ids.numel()
        s[W_ROWS] += int(ls.sum())
        ln[ids] = 0

    def _commit_all(self) -> None:
        self._commit(None, True)

    def _read_state(self):
        s = self.state
        count = min(int(s[W_COUNT]), self.desc_cap)
        return count, int(s[W_STATUS]), int(s[W_ROWS]), self._views()[3][:count].numpy().copy()

    def _gather(self, r0: int, m: int) -> list:
        desc = self._views()[3][:min(int(self.state[W_COUNT]), self.desc_cap)].long()
        r = torch.arange(r0, r0 + m)
        j = torch.searchsorted(desc[:, 3].contiguous(), r, right=True) - 1      # the last descriptor with offset <= r
        env, slot = desc[j, 0], (desc[j, 1] + r - desc[j, 3]) % self.R
        blocks = []
        for i, (_, _, _, rb, _) in enumerate(self.specs):
            out = self.out[i].view(self.piece, rb)
            out[:m] = self.stage[i].view(self.n, self.R, stage_pitch(rb))[env, slot, :rb]
            blocks.append(out[:m].reshape(-1).numpy().copy())
        return blocks

    def _drained(self) -> None:
        self.state[W_COUNT] = 0
        self.state[W_ROWS] = 0
        self._views()[2].zero_()


# ---------------------------------------------------------------------------------------------------------------- the kernels
class TraceCollector(_TraceBase):
    """The fused recorder: every tensor lives on ``device`` (default: the current ROCm device).  ``append`` is asynchronous on the
    current stream: two launches, no read-back, no host-written device memory.  ``calls`` logs every C entry point used, with its
    number of kernel launches."""

    def __init__(self, *args, device=None, **kw):
        _fused.require_gpu("TraceCollector", "TorchTraceCollector is the CPU model")
        self._lib = _lib.load()
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise ValueError("TraceCollector records on a ROCm device")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        super().__init__(*args, device=device, **kw)
        lib = self._lib
        for _, _, _, rb, _ in self.specs:
            assert lib.rover_trace_stage_pitch(rb) == stage_pitch(rb)
        assert lib.rover_trace_state_bytes(self.n, self.desc_cap) == state_bytes(self.n, self.desc_cap)
        self._streams = (_lib.TraceStream * len(self.specs))()
        for i, (_, _, _, rb, flags) in enumerate(self.specs):
            s = self._streams[i]
            s.stage, s.stage_pitch = self.stage[i].data_ptr(), stage_pitch(rb)
            s.out, s.out_pitch = self.out[i].data_ptr(), rb
            s.row_bytes, s.flags = rb, flags
        self._call("rover_trace_init", 0, self.state.data_ptr(), self.n, self.desc_cap)

    def _call(self, name: str, launches: int, *args) -> None:
        _fused.launch(name, self.device, *args)
        self.calls.append((name, launches))

    def _append(self, src, done) -> None:
        for i, (t, pitch) in enumerate(src):
            self._streams[i].src, self._streams[i].src_pitch = t.data_ptr(), pitch
        self._call("rover_trace_append", 2, self._streams, len(self.specs), self.state.data_ptr(), self.n, self.R, self.max_ep,
                   self.desc_cap, done.data_ptr())

    def _commit_all(self) -> None:
        self._call("rover_trace_commit_all", 1, self.state.data_ptr(), self.n, self.R, self.desc_cap)

    def _read_state(self):
        hdr = self.state[:HEADER_WORDS].cpu()                # the drain's one synchronisation
        count = min(int(hdr[W_COUNT]), self.desc_cap)
        d0 = desc_word(self.n)
        return count, int(hdr[W_STATUS]), int(hdr[W_ROWS]), self.state[d0:d0 + 4 * count].cpu().numpy().reshape(count, 4)

    def _gather(self, r0: int, m: int) -> list:
        self._call("rover_trace_gather", 1, self._streams, len(self.specs), self.state.data_ptr(), self.n, self.R, self.desc_cap, r0, m)
        return [self.out[i][:m * rb].cpu().numpy() for i, (_, _, _, rb, _) in enumerate(self.specs)]

    def _drained(self) -> None:
        self._call("rover_trace_drained", 1, self.state.data_ptr(), self.n)
