"""skrl's reward and episode curves, tracked on the MI355X (C ABI: ``include/rover_tracker.h``).

Every skrl agent writes, each ``write_interval`` steps, the max / min / mean of the instantaneous reward, of the total reward and
the length of the last 100 finished episodes, whatever ``track_data`` was fed (the reference's trainer feeds ``infos["episode"]``
as ``EpisodeInfo / ...``, rover_envs/utils/skrl_utils.py:138-142) and the agent's own ``Loss / ...`` scalars.  Three classes:

``SkrlTracking``         skrl 1.1.0's ``Agent.record_transition`` / ``track_data`` / ``write_tracking_data`` restated literally,
                         with ``collections.deque(maxlen=100)`` and numpy.  It synchronises with the host several times per step
                         when its tensors live on a GPU: it is what the other two are compared against, and what skrl costs.
``TorchEpisodeTracker``  the CPU specification of the kernels: the state block of ``rover_tracker.h`` word for word, every sum in
                         the order the header states, so that the device is compared with it bit for bit.
``EpisodeTracker``       the HIP kernels: two launches per env step, one per ``track`` / ``track_vector``, and one read-back per
                         write.  No CPU fallback.

What is not skrl's: skrl takes ``torch.mean(rewards)`` in float32 in whatever order torch adds; here the step's mean is a float64
sum in a fixed order, rounded to float32 once.  The windows' means are float64 sums from the oldest to the newest entry.  A tag must
be declared before it is tracked (its slot lives in device memory).
"""
from __future__ import annotations

import collections
import json
from typing import Callable, Iterable, Mapping, Sequence

import numpy as np
import torch

from . import _fused, _lib

WINDOW, CHUNK, HDR_WORDS, ACC_WORDS, MAX_SLOTS = 100, 256, 220, 20, 4096
W_N, W_SLOTS, W_HEAD, W_LEN, W_STEPS, W_WSTEPS, W_SUM, W_MAX, W_MIN, W_RING_R, W_RING_T = 0, 1, 2, 3, 4, 5, 8, 14, 17, 20, 120
BUILTIN_TAGS = tuple(f"{group} ({red})" for group in ("Reward / Instantaneous reward", "Reward / Total reward", "Episode / Total timesteps")
                     for red in ("max", "min", "mean"))
PPO_TAGS = ("Loss / Policy loss", "Loss / Value loss", "Policy / Standard deviation", "Learning / Learning rate")


def episode_info_tags(log_keys: Iterable[str]) -> tuple:
    """The tags the reference's trainer gives the entries of ``infos["episode"]`` (``envs.rover_env.LOG_KEYS`` are the leading words
    of ``RoverEnv.episode_log_vector``)."""
    return tuple(f"EpisodeInfo / {k}" for k in log_keys)


def reduction_of(tag: str) -> str:
    """skrl's ``write_tracking_data``: a tag that ends in ``(min)`` / ``(max)`` writes the min / max of its values, any other the mean."""
    return "min" if tag.endswith("(min)") else "max" if tag.endswith("(max)") else "mean"


class JsonlWriter:
    """A writer with TensorBoard's ``add_scalar(tag, value, step)``: one JSON object per line."""

    def __init__(self, path: str):
        self.path = path
        self._f = open(path, "w")

    def add_scalar(self, tag: str, value: float, step: int) -> None:
        self._f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")

    def flush(self) -> None:
        self._f.flush()

    def close(self) -> None:
        self._f.close()


# ---------------------------------------------------------------------------------------------------------------- skrl, literally
class SkrlTracking:
    """skrl 1.1.0's tracking, restated.  ``record_transition`` and ``track_data`` are the agent's; ``post_interaction`` is the part of
    the agent's that increments the timestep and writes.  ``clear_window_on_write``: whether ``write_tracking_data`` also clears the
    two deques."""

    def __init__(self, write_interval: int = 40, clear_window_on_write: bool = True, writer=None):
        self.write_interval = int(write_interval)
        self.clear_window_on_write = bool(clear_window_on_write)
        self.writer = writer
        self.tracking_data = collections.defaultdict(list)
        self._track_rewards = collections.deque(maxlen=WINDOW)
        self._track_timesteps = collections.deque(maxlen=WINDOW)
        self._cumulative_rewards = None
        self._cumulative_timesteps = None

    def track_data(self, tag: str, value: float) -> None:
        self.tracking_data[tag].append(value)

    def record_transition(self, rewards: torch.Tensor, terminated: torch.Tensor, truncated: torch.Tensor | None = None) -> None:
        if truncated is None:
            truncated = torch.zeros_like(terminated)
        if self._cumulative_rewards is None:
            self._cumulative_rewards = torch.zeros_like(rewards, dtype=torch.float32)
            self._cumulative_timesteps = torch.zeros_like(rewards, dtype=torch.int32)
        self._cumulative_rewards.add_(rewards)
        self._cumulative_timesteps.add_(1)
        finished_episodes = (terminated + truncated).reshape(-1).nonzero(as_tuple=False)
        if finished_episodes.numel():
            cr, ct = self._cumulative_rewards.view(-1), self._cumulative_timesteps.view(-1)
            self._track_rewards.extend(cr[finished_episodes][:, 0].reshape(-1).tolist())
            self._track_timesteps.extend(ct[finished_episodes][:, 0].reshape(-1).tolist())
            cr[finished_episodes] = 0
            ct[finished_episodes] = 0
        self.tracking_data["Reward / Instantaneous reward (max)"].append(torch.max(rewards).item())
        self.tracking_data["Reward / Instantaneous reward (min)"].append(torch.min(rewards).item())
        self.tracking_data["Reward / Instantaneous reward (mean)"].append(torch.mean(rewards).item())
        if len(self._track_rewards):
            track_rewards = np.array(self._track_rewards)
            track_timesteps = np.array(self._track_timesteps)
            self.tracking_data["Reward / Total reward (max)"].append(np.max(track_rewards))
            self.tracking_data["Reward / Total reward (min)"].append(np.min(track_rewards))
            self.tracking_data["Reward / Total reward (mean)"].append(np.mean(track_rewards))
            self.tracking_data["Episode / Total timesteps (max)"].append(np.max(track_timesteps))
            self.tracking_data["Episode / Total timesteps (min)"].append(np.min(track_timesteps))
            self.tracking_data["Episode / Total timesteps (mean)"].append(np.mean(track_timesteps))

    def write_tracking_data(self, timestep: int) -> dict:
        out = {}
        for k, v in self.tracking_data.items():
            if not len(v):
                continue
            out[k] = float(np.min(v) if k.endswith("(min)") else np.max(v) if k.endswith("(max)") else np.mean(v))
            if self.writer is not None:
                self.writer.add_scalar(k, out[k], timestep)
        if self.clear_window_on_write:
            self._track_rewards.clear()
            self._track_timesteps.clear()
        self.tracking_data.clear()
        return out

    def post_interaction(self, timestep: int):
        timestep += 1
        if timestep > 1 and self.write_interval > 0 and not timestep % self.write_interval:
            return self.write_tracking_data(timestep)
        return None


# ------------------------------------------------------------------------------------------------- what the two trackers share
def state_words(n: int, slots: int) -> int:
    """Mirror of ``rover_tracker_state_bytes`` / 4."""
    return HDR_WORDS + 6 * slots + 2 * n


def block_views(block: np.ndarray, n: int, slots: int) -> dict:
    """Typed numpy views of a state block (an int32 array of ``state_words`` words), by the names of ``rover_tracker.h``."""
    s0 = HDR_WORDS
    c0 = s0 + 6 * slots
    return {"head": block[W_HEAD:W_HEAD + 1], "len": block[W_LEN:W_LEN + 1], "steps": block[W_STEPS:W_STEPS + 1],
            "window_steps": block[W_WSTEPS:W_WSTEPS + 1], "sum": block[W_SUM:W_MAX].view(np.float64),
            "max": block[W_MAX:W_MIN].view(np.float32), "min": block[W_MIN:W_RING_R].view(np.float32),
            "ring_r": block[W_RING_R:W_RING_T].view(np.float32), "ring_t": block[W_RING_T:HDR_WORDS],
            "slot_sum": block[s0:s0 + 2 * slots].view(np.float64), "slot_count": block[s0 + 2 * slots:s0 + 4 * slots].view(np.int64),
            "slot_max": block[s0 + 4 * slots:s0 + 5 * slots].view(np.float32), "slot_min": block[s0 + 5 * slots:c0].view(np.float32),
            "cum_r": block[c0:c0 + n].view(np.float32), "cum_t": block[c0 + n:c0 + 2 * n]}


class _TrackerBase:
    """Tags, the write cadence and the arithmetic of a write: the same code reads the device's snapshot and the specification's."""

    def __init__(self, num_envs: int, tags: Sequence[str], write_interval: int, clear_window_on_write: bool, writer, callback):
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError("num_envs must be >= 1")
        self.tags = tuple(tags)
        if len(set(self.tags)) != len(self.tags) or set(self.tags) & set(BUILTIN_TAGS):
            raise ValueError("tags must be distinct and none of the nine built-in ones")
        if len(self.tags) > MAX_SLOTS:
            raise ValueError(f"at most {MAX_SLOTS} tags")
        self.slots = len(self.tags)
        self._slot = {t: i for i, t in enumerate(self.tags)}
        self.write_interval = int(write_interval)
        self.clear_window_on_write = bool(clear_window_on_write)
        self.writer = writer
        self.callback: Callable[[dict, int], None] | None = callback

    def slot_of(self, tag: str) -> int:
        try:
            return self._slot[tag]
        except KeyError:
            raise KeyError(f"tag {tag!r} was not declared in tags=") from None

    def _run_of(self, tags: Sequence[str]) -> int:
        first = self.slot_of(tags[0])
        if [self.slot_of(t) for t in tags] != list(range(first, first + len(tags))):
            raise ValueError("track_vector takes tags in the order they were declared, without gaps")
        return first

    def _finalise(self, snap: np.ndarray) -> dict:
        """The dict of a write from the words of a snapshot (``rover_tracker_snapshot``'s layout)."""
        s = self.slots
        steps, wsteps = int(snap[W_STEPS]), int(snap[W_WSTEPS])
        sums, mx, mn = snap[W_SUM:W_MAX].view(np.float64), snap[W_MAX:W_MIN].view(np.float32), snap[W_MIN:ACC_WORDS].view(np.float32)
        out = {}
        for g, count in enumerate((steps, wsteps, wsteps)):
            if count > 0:
                out[BUILTIN_TAGS[3 * g]] = float(mx[g])
                out[BUILTIN_TAGS[3 * g + 1]] = float(mn[g])
                out[BUILTIN_TAGS[3 * g + 2]] = float(sums[g] / np.float64(count))
        a = ACC_WORDS
        ssum, scnt = snap[a:a + 2 * s].view(np.float64), snap[a + 2 * s:a + 4 * s].view(np.int64)
        smx, smn = snap[a + 4 * s:a + 5 * s].view(np.float32), snap[a + 5 * s:a + 6 * s].view(np.float32)
        for i, tag in enumerate(self.tags):
            if scnt[i] > 0:
                red = reduction_of(tag)
                out[tag] = float(smn[i]) if red == "min" else float(smx[i]) if red == "max" else float(ssum[i] / np.float64(scnt[i]))
        return out

    def write(self, step: int) -> dict:
        data = self._finalise(self._snapshot())
        if self.writer is not None:
            for k, v in data.items():
                self.writer.add_scalar(k, v, step)
        if self.callback is not None:
            self.callback(data, step)
        return data

    def post_interaction(self, timestep: int):
        """skrl's ``post_interaction``: ``timestep`` is the loop's, the write is stamped ``timestep + 1``.  ``None`` unless it writes."""
        timestep += 1
        if timestep > 1 and self.write_interval > 0 and not timestep % self.write_interval:
            return self.write(timestep)
        return None

    def _meta(self) -> dict:
        return {"num_envs": self.num_envs, "tags": list(self.tags)}

    def _check_meta(self, sd: Mapping) -> np.ndarray:
        if int(sd["num_envs"]) != self.num_envs or list(sd["tags"]) != list(self.tags):
            raise ValueError("the checkpoint's tracker has other envs or tags")
        block = torch.as_tensor(sd["block"], dtype=torch.int32).reshape(-1)
        if block.numel() != state_words(self.num_envs, self.slots):
            raise ValueError("the checkpoint's tracker block has another size")
        return block


# ------------------------------------------------------------------------------------------------------------- the specification
def _max_nan(a, b):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a) | np.isnan(b), np.float32(np.nan), np.where(a > b, a, b)).astype(np.float32)


def _min_nan(a, b):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a) | np.isnan(b), np.float32(np.nan), np.where(a < b, a, b)).astype(np.float32)


def _add(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return a + b


def _tree(x: np.ndarray, op) -> np.ndarray:
    """x: (rows, 256); x[t] = op(x[t], x[t + s]) for s = 128 ... 1; returns column 0."""
    x = x.copy()
    s = CHUNK // 2
    while s:
        x[:, :s] = op(x[:, :s], x[:, s:2 * s])
        s >>= 1
    return x[:, 0]


def _fold(parts: np.ndarray, ident, op) -> np.generic:
    """Position t takes parts t, t + 256, ... in ascending order onto ``ident``, then the tree."""
    acc = np.full(CHUNK, ident, parts.dtype)
    for k in range(0, len(parts), CHUNK):
        m = min(CHUNK, len(parts) - k)
        acc[:m] = op(acc[:m], parts[k:k + m])
    return _tree(acc[None, :], op)[0]


def _flags(terminated, truncated, n: int) -> np.ndarray:
    """Finished envs: float flags as skrl adds them (in float32), byte flags or-ed."""
    def arr(x):
        x = x.detach().cpu() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
        x = x.reshape(-1)
        if x.numel() != n:
            raise ValueError(f"expected {n} flags")
        return x.numpy()
    t = arr(terminated)
    u = None if truncated is None else arr(truncated)
    if t.dtype == np.float32:
        if u is not None and u.dtype != np.float32:
            raise ValueError("terminated and truncated must have one dtype")
        with np.errstate(invalid="ignore"):
            return (t if u is None else t + u) != 0
    if t.dtype not in (np.bool_, np.uint8) or (u is not None and u.dtype not in (np.bool_, np.uint8)):
        raise ValueError("flags must be float32, bool or uint8")
    return (t != 0) if u is None else ((t != 0) | (u != 0))


class TorchEpisodeTracker(_TrackerBase):
    """The kernels of ``csrc/tracker_kernels.hip`` on the CPU: the same state block, the same reduction orders."""

    def __init__(self, num_envs: int, tags: Sequence[str] = (), write_interval: int = 40, clear_window_on_write: bool = True,
                 writer=None, callback=None):
        super().__init__(num_envs, tags, write_interval, clear_window_on_write, writer, callback)
        self.block = np.zeros(state_words(self.num_envs, self.slots), np.int32)
        self.block[W_N], self.block[W_SLOTS] = self.num_envs, self.slots
        self.v = block_views(self.block, self.num_envs, self.slots)
        for k in ("max", "slot_max"):
            self.v[k][:] = -np.inf
        for k in ("min", "slot_min"):
            self.v[k][:] = np.inf

    def step(self, rew, terminated, truncated=None) -> None:
        n, v = self.num_envs, self.v
        r = (rew.detach().cpu() if isinstance(rew, torch.Tensor) else torch.as_tensor(np.asarray(rew))).reshape(-1).numpy()
        if r.dtype != np.float32 or r.size != n:
            raise ValueError(f"rew must be {n} float32 values")
        fin = _flags(terminated, truncated, n)
        v["cum_r"][:] = _add(v["cum_r"], r)
        v["cum_t"] += 1
        # the chunks of 256 envs, then the chunk results
        nb = -(-n // CHUNK)
        pad = nb * CHUNK - n
        psum = _tree(np.concatenate([r.astype(np.float64), np.zeros(pad)]).reshape(nb, CHUNK), _add)
        pmax = _tree(np.concatenate([r, np.full(pad, -np.inf, np.float32)]).reshape(nb, CHUNK), _max_nan)
        pmin = _tree(np.concatenate([r, np.full(pad, np.inf, np.float32)]).reshape(nb, CHUNK), _min_nan)
        s_sum, s_max, s_min = _fold(psum, 0.0, _add), _fold(pmax, -np.inf, _max_nan), _fold(pmin, np.inf, _min_nan)
        # the finished envs into the windows
        ids = np.nonzero(fin)[0]
        K = len(ids)
        head, ln = int(v["head"][0]), int(v["len"][0])
        if K:
            rank = np.arange(K)
            keep = rank >= K - WINDOW
            slot = (head + rank[keep]) % WINDOW
            v["ring_r"][slot] = v["cum_r"][ids[keep]]
            v["ring_t"][slot] = v["cum_t"][ids[keep]]
            v["cum_r"][ids] = 0.0
            v["cum_t"][ids] = 0
        head, ln = (head + K) % WINDOW, min(WINDOW, ln + K)
        v["head"][0], v["len"][0] = head, ln
        v["steps"][0] += 1
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            v["sum"][0] = v["sum"][0] + np.float64(np.float32(s_sum / np.float64(n)))
        v["max"][0] = _max_nan(v["max"][0], s_max)
        v["min"][0] = _min_nan(v["min"][0], s_min)
        if ln > 0:
            order = (head - ln + np.arange(ln)) % WINDOW
            wr, wt = v["ring_r"][order], v["ring_t"][order]
            sr, st = np.float64(0.0), np.float64(0.0)
            rmx, rmn, tmx, tmn = np.float32(-np.inf), np.float32(np.inf), np.float32(-np.inf), np.float32(np.inf)
            for i in range(ln):                                    # oldest to newest
                sr, st = _add(sr, np.float64(wr[i])), st + np.float64(wt[i])
                rmx, rmn = _max_nan(rmx, wr[i]), _min_nan(rmn, wr[i])
                tmx, tmn = _max_nan(tmx, np.float32(wt[i])), _min_nan(tmn, np.float32(wt[i]))
            v["window_steps"][0] += 1
            v["sum"][1] = _add(v["sum"][1], sr / np.float64(ln))
            v["sum"][2] = v["sum"][2] + st / np.float64(ln)
            v["max"][1], v["min"][1] = _max_nan(v["max"][1], rmx), _min_nan(v["min"][1], rmn)
            v["max"][2], v["min"][2] = _max_nan(v["max"][2], tmx), _min_nan(v["min"][2], tmn)

    def _track(self, first: int, values: np.ndarray) -> None:
        v = self.v
        k = slice(first, first + len(values))
        v["slot_sum"][k] = _add(v["slot_sum"][k], values.astype(np.float64))
        v["slot_count"][k] += 1
        v["slot_max"][k] = _max_nan(v["slot_max"][k], values)
        v["slot_min"][k] = _min_nan(v["slot_min"][k], values)

    def track(self, tag: str, value) -> None:
        value = float(value.detach().cpu().reshape(-1)[0]) if isinstance(value, torch.Tensor) else float(value)
        with np.errstate(over="ignore"):
            self._track(self.slot_of(tag), np.array([value], np.float64).astype(np.float32))

    def track_vector(self, tags: Sequence[str], vector) -> None:
        first = self._run_of(tags)
        x = (vector.detach().cpu() if isinstance(vector, torch.Tensor) else torch.as_tensor(np.asarray(vector))).reshape(-1).numpy()
        if x.dtype != np.float32 or x.size < len(tags):
            raise ValueError("vector must hold at least len(tags) float32 values")
        self._track(first, x[:len(tags)])

    def _snapshot(self) -> np.ndarray:
        s, v = self.slots, self.v
        snap = np.concatenate([self.block[:ACC_WORDS], self.block[HDR_WORDS:HDR_WORDS + 6 * s]]).copy()
        for k in ("steps", "window_steps", "sum", "slot_sum", "slot_count"):
            v[k][:] = 0
        self.block[6:8] = 0
        for k in ("max", "slot_max"):
            v[k][:] = -np.inf
        for k in ("min", "slot_min"):
            v[k][:] = np.inf
        if self.clear_window_on_write:
            v["head"][0] = v["len"][0] = 0
        return snap

    def block_numpy(self) -> np.ndarray:
        return self.block.copy()

    def state_dict(self) -> dict:
        return {**self._meta(), "block": torch.from_numpy(self.block.copy())}

    def load_state_dict(self, sd: Mapping) -> None:
        self.block[:] = self._check_meta(sd).numpy()


# ---------------------------------------------------------------------------------------------------------------------- the device
class EpisodeTracker(_TrackerBase):
    """skrl's tracking as HIP kernels.  ``step`` is two launches, ``track`` / ``track_vector`` one, and nothing synchronises with
    the host until ``post_interaction`` reaches a write step: one launch that copies the accumulators out and clears them, and one
    device-to-host copy.  ``writer``: any object with ``add_scalar(tag, value, step)`` (``JsonlWriter``, a ``SummaryWriter``);
    ``callback(data, step)`` receives the dict of every write."""

    def __init__(self, num_envs: int, tags: Sequence[str] = (), write_interval: int = 40, clear_window_on_write: bool = True,
                 device="cuda", writer=None, callback=None):
        super().__init__(num_envs, tags, write_interval, clear_window_on_write, writer, callback)
        _fused.require_gpu("EpisodeTracker", "tracker.TorchEpisodeTracker is the specification")
        self._lib = _lib.load()
        nbytes = int(self._lib.rover_tracker_state_bytes(self.num_envs, self.slots))
        if nbytes != 4 * state_words(self.num_envs, self.slots):
            raise _lib.RoverHipError("rover_tracker_state_bytes of librover_hip.so does not match the Python mirror")
        self.state = torch.empty(nbytes // 4, dtype=torch.int32, device=torch.device(device))
        self.device = self.state.device
        self.ws = torch.empty(int(self._lib.rover_tracker_workspace_bytes(self.num_envs)), dtype=torch.uint8, device=self.device)
        self._snap = torch.empty(int(self._lib.rover_tracker_snapshot_words(self.slots)), dtype=torch.int32, device=self.device)
        _lib.check(self._lib.rover_tracker_init(self.state.data_ptr(), self.num_envs, self.slots, self._stream()), "rover_tracker_init")

    def _stream(self):
        return _fused.stream(self.device)

    def _vec(self, x: torch.Tensor, name: str, dtypes, numel: int | None = None) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.device != self.device or x.dtype not in dtypes:
            raise ValueError(f"{name} must be a cuda tensor on the tracker's device of dtype {' / '.join(str(d) for d in dtypes)}")
        x = x.reshape(-1)
        if not x.is_contiguous() or (numel is not None and x.numel() != numel):
            raise ValueError(f"{name} must hold {numel} contiguous values")
        return x

    @torch.no_grad()
    def step(self, rew: torch.Tensor, terminated: torch.Tensor, truncated: torch.Tensor | None = None) -> None:
        """One env step: ``rew`` float32 ``(n,)`` or ``(n, 1)``; the flags float32 (as the collectors hold them) or bool / uint8 (as
        the envs return them), both of one dtype; ``truncated`` may be None."""
        n = self.num_envs
        flag_types = (torch.float32, torch.bool, torch.uint8)
        rew = self._vec(rew, "rew", (torch.float32,), n)
        terminated = self._vec(terminated, "terminated", flag_types, n)
        if truncated is not None:
            truncated = self._vec(truncated, "truncated", flag_types, n)
            if truncated.element_size() != terminated.element_size():
                raise ValueError("terminated and truncated must have one dtype")
        _lib.check(self._lib.rover_tracker_step(self.state.data_ptr(), n, self.slots, rew.data_ptr(), terminated.data_ptr(),
                                                None if truncated is None else truncated.data_ptr(), terminated.element_size(),
                                                self.ws.data_ptr(), self.ws.numel(), self._stream()), "rover_tracker_step")

    def _track(self, first: int, values: torch.Tensor, count: int) -> None:
        _lib.check(self._lib.rover_tracker_track(self.state.data_ptr(), self.num_envs, self.slots, first, values.data_ptr(), count,
                                                 self._stream()), "rover_tracker_track")

    @torch.no_grad()
    def track(self, tag: str, value) -> None:
        """``track_data``: a float32 device tensor of one element is read where it lies (no read-back); a Python number is copied
        to the device first."""
        slot = self.slot_of(tag)
        if not isinstance(value, torch.Tensor):
            value = torch.tensor([float(value)], dtype=torch.float32).to(self.device, non_blocking=True)
        self._track(slot, self._vec(value, "value", (torch.float32,), 1), 1)

    @torch.no_grad()
    def track_vector(self, tags: Sequence[str], vector: torch.Tensor) -> None:
        """``track_data(tags[i], vector[i])`` for every i in one launch: ``tags`` in their declared order, ``vector`` a float32
        device tensor of at least ``len(tags)`` values (the env's log vector)."""
        first = self._run_of(tags)
        vector = self._vec(vector, "vector", (torch.float32,))
        if vector.numel() < len(tags):
            raise ValueError("vector must hold at least len(tags) values")
        self._track(first, vector, len(tags))

    def _snapshot(self) -> np.ndarray:
        _lib.check(self._lib.rover_tracker_snapshot(self.state.data_ptr(), self.num_envs, self.slots, self._snap.data_ptr(),
                                                    int(self.clear_window_on_write), self._stream()), "rover_tracker_snapshot")
        return self._snap.cpu().numpy()                          # the one synchronisation of a write interval

    def block_numpy(self) -> np.ndarray:
        """The state block on the host (``block_views`` names its parts).  Synchronises."""
        return self.state.cpu().numpy()

    def state_dict(self) -> dict:
        return {**self._meta(), "block": self.state.cpu()}

    def load_state_dict(self, sd: Mapping) -> None:
        self.state.copy_(self._check_meta(sd).to(self.device))


def add_arguments(ap) -> None:
    """The examples' ``--track [PATH]`` and ``--write_interval N``."""
    ap.add_argument("--track", nargs="?", const="-", default=None, metavar="PATH",
                    help="track skrl's reward / episode curves on the device (isaac_rover_orbit_amd.tracker) and write them every "
                         "--write_interval steps: JSON lines into PATH, or one {\"tracking\": ...} line on stdout without PATH")
    ap.add_argument("--write_interval", type=int, default=40, metavar="N", help="skrl's write_interval (40 in the rover's agent files)")


def from_args(args, num_envs: int, tags: Sequence[str] = (), device="cuda"):
    """The ``EpisodeTracker`` ``--track`` asks for, or None."""
    if args.track is None:
        return None
    if args.track == "-":
        return EpisodeTracker(num_envs, tags, args.write_interval, device=device,
                              callback=lambda data, step: print(json.dumps({"tracking": data, "step": step}), flush=True))
    writer = JsonlWriter(args.track)
    return EpisodeTracker(num_envs, tags, args.write_interval, device=device, writer=writer, callback=lambda data, step: writer.flush())


def track_ppo_update(tracker, trainer, epochs: int | None = None, minibatches: int | None = None) -> None:
    """skrl PPO's scalars of one update, from what ``ppo.FusedPPO.update`` left on the device: ``last_stats`` ``(epochs, minibatches,
    4)`` holds KL, policy loss and value loss per minibatch (NaN where the KL early stop skipped one).  As in skrl the losses are the
    sums over the minibatches that ran divided by ``epochs * minibatches``.  A few small torch kernels per update and no read-back."""
    trainer = getattr(trainer, "inner", trainer)                 # ppo_scaled.FusedScaledPPO wraps the FusedPPO that holds them
    stats = trainer.last_stats
    e = stats.shape[0] if epochs is None else epochs
    m = stats.shape[1] if minibatches is None else minibatches
    sums = torch.nansum(stats.reshape(-1, stats.shape[-1])[:, 1:3], dim=0) / float(e * m)
    tracker.track("Loss / Policy loss", sums[0:1])
    tracker.track("Loss / Value loss", sums[1:2])
    tracker.track("Policy / Standard deviation", trainer.log_std.detach().exp().mean().reshape(1).float())
    tracker.track("Learning / Learning rate", trainer.state[:1].to(torch.float32))
