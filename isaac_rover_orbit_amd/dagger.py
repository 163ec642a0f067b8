"""DAgger: distil the rover's privileged policy into a 31 x 31 depth student (C ABI: ``include/rover_dagger.h``).

The reference's ``RoverEnvCamera`` exists for "collecting camera data for Learning By Cheating": a teacher drives from the 961-ray
height scan, a student learns to drive from what the on-board camera sees.  At ``CameraCfg(width=31, height=31)`` the depth image has
961 pixels, the width of the height scan, so the student is the reference's own policy network on a 965-wide *student row* whose scan
columns hold depth -- ``RoverNet``, checkpoint conversion and ``examples/03_eval_policy.py``'s actor loading apply unchanged.

    row[:, 0:4]   = nan_to_num(env_row[:, 0:4])                        last action, distance, heading
    row[:, 4 + p] = depth_scale * min(d_p, depth_clip)                 p row-major over the (height, width) render buffer;
                                                                       a NaN, +-inf or negative pixel counts as depth_clip

The encoder reads columns [3, 964) (the reference's slice, models.py:95): the heading plus the first 960 pixels; the last pixel is
stored and never read.

The loop (Ross et al. 2011), around ``env.step`` and with a ``td3.ReplayMemory`` as the aggregated dataset (the observation ring holds
student rows, the action slot holds the teacher's label a*)::

    col.begin(obs, env.extras["depth"])                       # rows after reset -> ring[cursor]
    loop:
        a = col.act(beta)                                      # a* and a_s; env i takes a* if u_i < beta else a_s; a* -> memory
        obs, rew, term, trunc, info = env.step(a)
        idx = col.record(obs, env.extras["depth"], rew, term, batch_size=B)
        trainer.update(memory, idx)                            # L = (1 / 2B) sum (tanh(z) - a*)^2, Adam, replicas

``beta`` is an argument of every ``act``: the host owns the schedule.  The draw ``u`` is counter-based (Philox4x32-10 keyed by the seed,
indexed by global env id and counter), so it does not depend on how the envs are split over ranks and the checkpoint is the counter.

``TorchDAgger`` / ``TorchDAggerCollector`` are the specification in torch / numpy (CPU, any dtype); ``FusedDAgger`` / ``DAggerCollector``
run the HIP kernels.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping

import numpy as np
import torch
import torch.nn as nn

from . import _fused, _lib
from ._fused import f32_cuda, holds, launch, ptr
from .cfg import CameraCfg
from .ppo import pack, unpack
from .rollout import FLT_MAX
from .td3 import ACT_DIM, OBS_DIM, ReplayMemory
from .td3_collect import _CollectorBase, sample_indices
from .td3_explore import random_uniforms

SIDE, PIXELS, PROP = 31, 961, 4
# depth_clip / depth_scale: metres and the factor that brings a clipped pixel into [0, 1]; lr and Adam are torch's defaults
HPARAMS = dict(depth_clip=10.0, depth_scale=0.1, learning_rate=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, grad_norm_clip=0.0)
LOG_STD_KEY = "log_std_parameter"


def student_camera_cfg() -> CameraCfg:
    """The reference's camera (mount, lens, clip range) at 31 x 31 pixels."""
    return CameraCfg(width=SIDE, height=SIDE)


def image_buffer(depth: torch.Tensor) -> torch.Tensor:
    """(n, 961): the render buffer behind ``depth``, without a copy.  ``depth`` is the buffer itself ((n, 961) or (n, height, width),
    contiguous) or the env's ``extras["depth"]``, the (n, width, height) permuted view of it."""
    if depth.dim() == 3 and not depth.is_contiguous() and depth.permute(0, 2, 1).is_contiguous():
        depth = depth.permute(0, 2, 1)
    if not depth.is_contiguous() or depth.dim() not in (2, 3) or depth[0].numel() != PIXELS:
        raise ValueError(f"depth must be extras['depth'] of a {SIDE} x {SIDE} camera or its contiguous (n, {SIDE}, {SIDE}) buffer")
    return depth.reshape(depth.shape[0], PIXELS)


def sanitise(rows: torch.Tensor) -> torch.Tensor:
    """The off-policy collectors' rule for env rows."""
    return torch.nan_to_num(rows, nan=0.0, posinf=FLT_MAX, neginf=0.0)


def depth_pixels(d: torch.Tensor, depth_clip: float, depth_scale: float) -> torch.Tensor:
    """The pixel rule, in the dtype of ``d``: ``depth_scale * min(d, depth_clip)``, where a NaN, +-inf or negative pixel counts as
    ``depth_clip``.  One product per pixel."""
    clip = torch.tensor(depth_clip, dtype=d.dtype, device=d.device)
    scale = torch.tensor(depth_scale, dtype=d.dtype, device=d.device)
    d = torch.where(torch.isnan(d) | torch.isinf(d) | (d < 0), clip, d)
    return scale * torch.minimum(d, clip)


def student_rows(depth: torch.Tensor, env_rows: torch.Tensor, depth_clip: float = HPARAMS["depth_clip"],
                 depth_scale: float = HPARAMS["depth_scale"]) -> torch.Tensor:
    """The student rows (n, 965) in the dtype of ``env_rows``: the specification of ``rover_dagger_rows``."""
    x = depth_pixels(image_buffer(depth).to(env_rows.dtype), depth_clip, depth_scale)
    return torch.cat([sanitise(env_rows[:, :PROP]), x], dim=1)


def mix_uniforms(seed: int, env_ids, counter: int) -> np.ndarray:
    """float32 u (len(env_ids),) inside (0, 1): column 0 of ``td3_explore.random_uniforms``, the stream of the TD3 explorer's random
    steps (word 0 of Philox4x32-10((g, counter_lo, counter_hi, td3_explore.RANDOM_TAG), key = seed)), reused as it stands."""
    return random_uniforms(seed, env_ids, counter, 1)[:, 0]


def imitation_loss(actions: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """L = (1 / 2B) sum (a - a*)^2 over (B, 2)."""
    return ((actions - labels) ** 2).sum() / (2 * actions.shape[0])


def imitation_dz(actions: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """dL/dz in closed form for a = tanh(z): (a - a*) (1 - a^2) / B."""
    return (actions - labels) * (1 - actions * actions) / actions.shape[0]


def _hparams(overrides: Mapping) -> dict:
    hp = dict(HPARAMS)
    for k, v in overrides.items():
        if k not in hp:
            raise TypeError(f"unknown hyper-parameter {k!r}")
        hp[k] = v
    return hp


# ---------------------------------------------------------------------------------------------------------------- torch spec
class TorchDAgger:
    """One imitation step in torch autograd on the student (``Net(2, True)`` of examples/04_train_ppo.py: it returns tanh(z)); any
    dtype (the tests run float64)."""

    def __init__(self, student: nn.Module, **hparams):
        self.hp = _hparams(hparams)
        self.student = student
        params = [p for k, p in student.named_parameters() if k != LOG_STD_KEY]
        self.optimizer = torch.optim.Adam(params, lr=self.hp["learning_rate"], betas=(self.hp["beta1"], self.hp["beta2"]),
                                          eps=self.hp["eps"])
        self._params = params

    @property
    def dtype(self):
        return self._params[0].dtype

    def act(self, rows):
        with torch.no_grad():
            return self.student(rows)

    def step(self, rows: torch.Tensor, labels: torch.Tensor) -> dict:
        """One step on given rows (B, 965) and labels (B, 2); returns loss, grad_norm (before clipping) and the closed-form dz."""
        a = self.student(rows)
        loss = imitation_loss(a, labels)
        self.optimizer.zero_grad()
        loss.backward()
        norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in self._params]))
        if self.hp["grad_norm_clip"] > 0:
            nn.utils.clip_grad_norm_(self._params, self.hp["grad_norm_clip"])
        self.optimizer.step()
        return {"loss": float(loss.detach()), "grad_norm": float(norm), "dz": imitation_dz(a.detach(), labels)}

    def update(self, memory: ReplayMemory, idx: torch.Tensor) -> dict:
        """One step on the rows ``idx`` of ``memory``: its states are student rows, its actions the labels."""
        s, a, _, _, _ = memory.gather(idx)
        return self.step(s.to(self.dtype), a.to(self.dtype))

    def checkpoint(self) -> dict:
        """``{"policy": state_dict}``: what ``RoverNet.from_checkpoint(role="policy")`` loads."""
        return {"policy": {k: v.detach().clone() for k, v in self.student.state_dict().items()}}


class _DaggerCollectorBase(_CollectorBase):
    def __init__(self, memory: ReplayMemory, seed: int, env_id_offset: int, depth_clip: float, depth_scale: float):
        super().__init__(memory, seed, env_id_offset, 0.0, (-1.0, 1.0), None)
        if self.A != ACT_DIM:
            raise ValueError("the memory must hold 2-wide actions")
        self.depth_clip, self.depth_scale = float(depth_clip), float(depth_scale)
        if not (0 < self.depth_clip < float("inf")):
            raise ValueError("depth_clip must be positive and finite")

    _image_buffer = staticmethod(image_buffer)                    # the camera's: dagger_conv's collectors set their own

    def _image(self, depth) -> torch.Tensor:
        d = self._image_buffer(depth)
        if d.shape[0] != self.n or d.dtype != torch.float32 or d.device != self.memory.obs.device:
            raise ValueError(f"depth must hold {self.n} float32 images on {self.memory.obs.device}")
        return d

    @staticmethod
    def _beta(beta) -> float:
        beta = float(np.float32(beta))
        if not 0.0 <= beta <= 1.0:
            raise ValueError("beta must lie in [0, 1]")
        return beta


class TorchDAggerCollector(_DaggerCollectorBase):
    """The specification, in torch / numpy.  ``teacher`` / ``student``: callables (n, 965) -> (n, 2) returning the tanh mean.
    ``last`` keeps the step's label, student action and chosen source (1 = teacher)."""

    def __init__(self, teacher, student, memory: ReplayMemory, seed: int = 42, env_id_offset: int = 0,
                 depth_clip: float = HPARAMS["depth_clip"], depth_scale: float = HPARAMS["depth_scale"]):
        super().__init__(memory, seed, env_id_offset, depth_clip, depth_scale)
        self.teacher, self.student = teacher, student
        self.teacher_rows = None
        self.last: dict = {}

    def draws(self, counter: int | None = None) -> np.ndarray:
        """float64 u (n,) of ``counter`` (default: the next call's)."""
        ids = self.env_id_offset + np.arange(self.n, dtype=np.int64)
        return mix_uniforms(self.seed, ids, self.counter if counter is None else counter)

    def _rows(self, raw, depth, slot: int) -> None:
        self.memory.obs[slot] = student_rows(self._image(depth), raw, self.depth_clip, self.depth_scale)
        self.teacher_rows = sanitise(raw)

    @torch.no_grad()
    def begin(self, raw_obs, depth) -> None:
        m = self.memory
        self._rows(self._raw(raw_obs), depth, m.cursor)
        m._last_next, m._last_version = None, -1

    @torch.no_grad()
    def act(self, beta: float) -> torch.Tensor:
        m = self.memory
        beta = self._beta(beta)
        label = self.teacher(self.teacher_rows)
        a_s = self.student(m.obs[m.cursor])
        source = torch.from_numpy(self.draws() < beta).to(label.device)
        a = torch.where(source.unsqueeze(1), label, a_s)
        m.actions[m.memory_index] = label
        self.last = {"label": label, "student": a_s, "source": source}
        self.counter += 1
        return a

    @torch.no_grad()
    def record(self, raw_obs, depth, rew, terminated, batch_size: int | None = None):
        m = self.memory
        raw = self._raw(raw_obs)
        self._transition(rew, terminated)
        k, w = m.memory_index, m.cursor
        self._rows(raw, depth, (w + 1) % m.slots)
        m.rewards[k] = rew.reshape(self.n)
        m.terminated[k] = terminated.reshape(self.n) != 0
        m.ring_pos[k] = w
        self._advance()
        idx = None
        if batch_size is not None:
            idx = torch.from_numpy(sample_indices(self.seed, self.counter, batch_size, len(m))).to(m.device)
        self.counter += 1
        return idx


# ---------------------------------------------------------------------------------------------------------------- fused
def default_hparams() -> "_lib.DaggerHparams":
    return _fused.default_hparams(_lib.DaggerHparams, "rover_dagger_default_hparams")


def _collector_hparams(seed: int, env_id_offset: int, depth_clip: float, depth_scale: float) -> "_lib.DaggerHparams":
    hp = _fused.seeded(default_hparams(), seed, env_id_offset)
    hp.depth_clip, hp.depth_scale = depth_clip, depth_scale
    return hp


def fused_student_rows(depth: torch.Tensor, env_rows: torch.Tensor, out: torch.Tensor | None = None, teacher_rows_out=None,
                       depth_clip: float = HPARAMS["depth_clip"], depth_scale: float = HPARAMS["depth_scale"]) -> torch.Tensor:
    """One ``rover_dagger_rows`` launch on the current stream: ``student_rows`` on the device (bit for bit), optionally with the
    sanitised env rows the teacher reads."""
    _fused.require_gpu("fused_student_rows", "student_rows is the CPU specification")
    d = image_buffer(depth)
    n = int(env_rows.shape[0])
    if out is None:
        out = torch.empty(n, OBS_DIM, dtype=torch.float32, device=env_rows.device)
    for name, t in (("depth", d), ("env_rows", env_rows), ("out", out), ("teacher_rows_out", teacher_rows_out)):
        f32_cuda(name, t, env_rows.device, "the rows' device")
    holds("depth", d, (n, PIXELS))
    for name, t in (("env_rows", env_rows), ("out", out), ("teacher_rows_out", teacher_rows_out)):
        holds(name, t, (n, OBS_DIM))
    launch("rover_dagger_rows", env_rows.device, C.byref(_collector_hparams(0, 0, depth_clip, depth_scale)), d.data_ptr(),
           env_rows.data_ptr(), n, out.data_ptr(), ptr(teacher_rows_out))
    return out


class FusedDAgger(_fused.FusedOffPolicy):
    """DAgger trainer state on the GPU: the student's packed parameters, Adam's moments and the device state struct
    (rover_dagger_state).  ``update`` runs one imitation step without a host synchronisation; ``stats`` reads the state (one
    synchronisation).  ``.actor`` aliases the student (a tanh ``RoverNet`` on replicas that every update refreshes)."""

    _STATE, _WORKSPACE, _PARAM_FLOATS = _lib.DaggerState, "rover_dagger_workspace_bytes", "rover_dagger_param_floats"
    _RUNS = "the reference policy network (Net(2, True)) only (rover_dagger.h)"
    _unpack = staticmethod(unpack)
    _CONVERT = {"learning_rate": "lr"}

    def __init__(self, student_sd: Mapping[str, torch.Tensor], device="cuda", n_copies: int = 4, **hparams):
        hparams = {self._CONVERT.get(k, k): v for k, v in hparams.items()}
        super().__init__(default_hparams, hparams, device, n_copies)
        self.desc_a, pa = pack(student_sd, "tanh")
        self.desc_c = None
        self.P = int(getattr(self._lib, self._PARAM_FLOATS)(C.byref(self.desc_a)))
        if self.P == 0:
            raise _lib.RoverHipError(f"{type(self).__name__} runs {self._RUNS}")
        self.n_a, self.n_c = pa.size, 0
        self._alloc(self._flat(pa))
        self.state = torch.zeros(C.sizeof(_lib.DaggerState) // 4, dtype=torch.int32, device=self.device)

    def _flat(self, pa: np.ndarray) -> np.ndarray:
        """The initial vector of ``P`` floats: the packed student, then zeros."""
        return np.concatenate([pa, np.zeros(self.P - pa.size, np.float32)])

    @staticmethod
    def _checkpoint_args(ck):
        return (ck["policy"],)

    def blocks(self, vec: torch.Tensor) -> dict:
        return {"policy": vec[:self.n_a]}

    # ---- views
    def checkpoint(self) -> dict:
        """``{"policy": state_dict}`` that ``Net(2, True)`` and ``RoverNet.from_checkpoint(role="policy")`` load (float32 CPU)."""
        sd = self.unvector(self.params)["policy"]
        sd[LOG_STD_KEY] = torch.zeros(ACT_DIM)
        return {"policy": sd}

    def state_dict(self) -> dict:
        """The checkpoint plus what a resumed run needs to continue bit for bit: the packed vectors and the device state."""
        sd = self.checkpoint()
        sd["dagger"] = {k: getattr(self, k).detach().cpu().clone() for k in ("params", "adam_m", "adam_v", "state")}
        return sd

    def load_state_dict(self, sd: dict) -> None:
        for k, v in sd["dagger"].items():
            getattr(self, k).copy_(v)
        self.rep_a.copy_(self.params[:self.n_a].repeat(self.n_copies))

    # ---- kernels
    def update(self, memory: ReplayMemory, idx: torch.Tensor, dz_out: torch.Tensor | None = None) -> None:
        """One imitation step on rows ``idx`` of ``memory`` (no host synchronisation)."""
        n = self._sample(memory, idx)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rover_dagger_update(
                C.byref(self.desc_a), C.byref(self.hp), self.params.data_ptr(), self.grad.data_ptr(), self.adam_m.data_ptr(),
                self.adam_v.data_ptr(), memory.obs.data_ptr(), memory.slots, memory.num_envs, memory.ring_pos.data_ptr(),
                memory.actions.data_ptr(), idx.data_ptr(), n, len(memory), self.ws.data_ptr(), self.ws.numel(), self.state.data_ptr(),
                self.rep_a.data_ptr(), self.n_copies, self._out(dz_out, 2 * n, "dz_out"), self._stream()), "rover_dagger_update")


class DAggerCollector(_DaggerCollectorBase):
    """The fused collector: ``teacher`` and ``student`` are tanh ``RoverNet``s (reference architecture, two outputs) and ``memory`` a
    ``ReplayMemory`` on the same device, all held BY REFERENCE -- with ``FusedDAgger.actor`` as the student the collector always sees
    the trainer's current parameters.  ``act`` returns a buffer the next call overwrites, ``record`` likewise (one index buffer per
    batch size).  ``begin`` and ``record`` are one launch each, ``act`` two (the teacher, then the student with the mix)."""

    def __init__(self, teacher, student, memory: ReplayMemory, seed: int = 42, env_id_offset: int = 0,
                 depth_clip: float = HPARAMS["depth_clip"], depth_scale: float = HPARAMS["depth_scale"]):
        _fused.require_gpu("DAggerCollector", "TorchDAggerCollector is the CPU specification")
        super().__init__(memory, seed, env_id_offset, depth_clip, depth_scale)
        self.teacher, self.student = teacher, student
        dev = memory.obs.device
        for net in (teacher, student):
            if net.packed.device != dev or net.out_dim != ACT_DIM:
                raise ValueError("teacher and student must live on the memory's device and have 2 outputs")
        self.teacher_rows = torch.zeros(self.n, OBS_DIM, dtype=torch.float32, device=dev)
        self._env_act = torch.zeros(self.n, ACT_DIM, dtype=torch.float32, device=dev)
        self._bufs: dict = {}

    def hparams(self) -> "_lib.DaggerHparams":
        return _collector_hparams(self.seed, self.env_id_offset, self.depth_clip, self.depth_scale)

    def _record(self, raw, depth, ring_slot, counter=0, idx=None, rew=None, terminated=None, rew_out=None, term_out=None,
                ring_pos_entry=None, ring_pos_value=0, mem_rows=0) -> None:
        launch("rover_dagger_record", raw.device, C.byref(self.hparams()), self._image(depth).data_ptr(), raw.data_ptr(), self.n,
               ring_slot.data_ptr(), self.teacher_rows.data_ptr(), ptr(rew), ptr(terminated), ptr(rew_out), ptr(term_out),
               ptr(ring_pos_entry), int(ring_pos_value), ptr(idx), 0 if idx is None else int(idx.numel()), int(mem_rows),
               C.c_uint64(int(counter)))

    @torch.no_grad()
    def begin(self, raw_obs, depth) -> None:
        """The rows after a reset go into the ring's cursor slot (and the teacher's scratch rows).  No draw: the counter stays.  A
        resumed run calls it with the env's current rows before its first ``act``."""
        m = self.memory
        self._record(self._raw(raw_obs), depth, m.obs[m.cursor])
        m._last_next, m._last_version = None, -1

    @torch.no_grad()
    def act(self, beta: float, student_out=None, source_out=None) -> torch.Tensor:
        """Teacher and student on the cursor slot; the label goes to the memory's action slot, the mixed actions are returned for
        ``env.step``.  ``student_out`` (n, 2) float32 / ``source_out`` (n,) uint8 receive a_s and the chosen source (1 = teacher).
        Advances the counter by one."""
        m = self.memory
        beta = self._beta(beta)
        dev = m.obs.device
        f32_cuda("student_out", student_out, dev, "the memory's device")
        holds("student_out", student_out, (self.n, ACT_DIM))
        if source_out is not None and (not source_out.is_cuda or source_out.dtype != torch.uint8 or not source_out.is_contiguous()
                                       or source_out.numel() != self.n or source_out.device != dev):
            raise ValueError(f"source_out must be a contiguous uint8 cuda tensor of {self.n} elements")
        t, s = self.teacher, self.student
        launch("rover_dagger_act", dev, C.byref(t.desc), t.packed.data_ptr(), t.n_copies, C.byref(s.desc), s.packed.data_ptr(),
               s.n_copies, C.byref(self.hparams()), C.c_uint64(int(self.counter)), C.c_float(beta), self.teacher_rows.data_ptr(),
               m.obs[m.cursor].data_ptr(), self.n, m.actions[m.memory_index].data_ptr(), self._env_act.data_ptr(), ptr(student_out),
               ptr(source_out))
        self.counter += 1
        return self._env_act

    @torch.no_grad()
    def record(self, raw_obs, depth, rew: torch.Tensor, terminated: torch.Tensor, batch_size: int | None = None):
        """The transition of the step just taken: the student rows of the env's new state into the next ring slot, reward / terminated
        / ring_pos of memory slot k; with ``batch_size`` the int64 row indices of a batch over the memory INCLUDING this transition,
        else ``None``.  Advances the memory as ``ReplayMemory.add`` does, and the counter by one."""
        m = self.memory
        raw = self._raw(raw_obs)
        self._transition(rew, terminated)
        if not rew.is_cuda:
            raise ValueError("rew and terminated must be cuda tensors")
        if batch_size is not None and int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        k, w = m.memory_index, m.cursor
        self._advance()
        idx = None
        if batch_size is not None:
            batch = int(batch_size)
            if batch not in self._bufs:
                self._bufs[batch] = torch.zeros(batch, dtype=torch.int64, device=m.obs.device)
            idx = self._bufs[batch]
        self._record(raw, depth, m.obs[(w + 1) % m.slots], self.counter, idx, rew=rew, terminated=terminated, rew_out=m.rewards[k],
                     term_out=m.terminated[k], ring_pos_entry=m.ring_pos[k:k + 1], ring_pos_value=w, mem_rows=len(m))
        self.counter += 1
        return idx
