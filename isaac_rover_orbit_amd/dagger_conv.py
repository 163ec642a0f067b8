"""DAgger at the camera the reference defines: a learned convolutional stem in front of the depth student (C ABI:
``include/rover_dagger_conv.h``).

``dagger.py`` distils the privileged policy into a student that reads a 31 x 31 camera, because 961 pixels fit the reference network's
scan input with nothing in between.  ``RoverEnvCamera``'s camera is 160 x 90.  Here the student reads that image through a small stem,
trained end to end with the unchanged reference network behind it::

    x        = depth_scale * min(d, depth_clip)                  d = depth_clip where the pixel is NaN, +-inf or negative (dagger.py's rule)
    h        = LeakyReLU_0.01(Conv2d(1 -> 8, kernel (6, 10), stride (3, 5), padding (3, 0))(x))        (n, 8, 31, 31)
    y        = Conv2d(8 -> 1, kernel 1)(h)                                                             (n, 31, 31)
    row[:, 4 + 31 i + j] = y[:, i, j];   row[:, 0:4] = nan_to_num(env_row[:, 0:4])

The stem has 497 parameters, packed as ``W1[8][6][10], b1[8], w2[8], b2``.  The encoder reads columns [3, 964) (models.py:95), so
feature (30, 30) is computed, stored and never read and its gradient is exactly 0.

Everything else is ``dagger.py``'s: teacher, label, the Philox mixing draw, ``rover_dagger_act``, a ``td3.ReplayMemory`` as the dataset,
the imitation loss, clip / Adam / replicas.  Beside the memory an ``ImageRing`` keeps the preprocessed images, addressed by the memory's
own ring row number: the update recomputes the features of the sampled rows under the stem's current parameters.

``ConvStem`` / ``conv_student_rows`` / ``TorchConvDAgger`` / ``TorchConvDAggerCollector`` are the specification in torch (CPU, any dtype);
``FusedConvDAgger`` / ``ConvDAggerCollector`` run the HIP kernels.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _fused, _lib
from ._fused import f32_cuda, holds, launch, ptr
from .cfg import CameraCfg
from .dagger import (HPARAMS, LOG_STD_KEY, DAggerCollector, FusedDAgger, TorchDAggerCollector, _DaggerCollectorBase, _collector_hparams,
                     _hparams, depth_pixels, imitation_dz, imitation_loss, mix_uniforms, sanitise)  # noqa: F401 (mix_uniforms: re-export)
from .td3 import OBS_DIM, ReplayMemory

IMG_H, IMG_W, PIXELS = 90, 160, 14400
SIDE, FEATURES, PROP = 31, 961, 4
CHANNELS, KERNEL, STRIDE, PADDING, SLOPE = 8, (6, 10), (3, 5), (3, 0), 0.01
TAPS = KERNEL[0] * KERNEL[1]
STEM_FLOATS = CHANNELS * TAPS + CHANNELS + CHANNELS + 1          # 497
STEM_KEY = "student_stem"


def student_camera_cfg() -> CameraCfg:
    """The reference's camera as it stands: 160 x 90."""
    return CameraCfg()


def image_buffer(depth: torch.Tensor) -> torch.Tensor:
    """(n, 90, 160): the render buffer behind ``depth``, without a copy.  ``depth`` is the buffer itself ((n, 14400) or (n, 90, 160),
    contiguous) or the env's ``extras["depth"]``, the (n, 160, 90) permuted view of it.  Any other image size is refused."""
    if depth.dim() == 3 and not depth.is_contiguous() and depth.permute(0, 2, 1).is_contiguous():
        depth = depth.permute(0, 2, 1)
    ok = depth.is_contiguous() and ((depth.dim() == 2 and depth.shape[1] == PIXELS) or
                                    (depth.dim() == 3 and tuple(depth.shape[1:]) == (IMG_H, IMG_W)))
    if not ok:
        raise ValueError(f"depth must be extras['depth'] of a {IMG_W} x {IMG_H} camera or its contiguous (n, {IMG_H}, {IMG_W}) buffer")
    return depth.reshape(depth.shape[0], IMG_H, IMG_W)


def preprocess(depth: torch.Tensor, depth_clip: float = HPARAMS["depth_clip"], depth_scale: float = HPARAMS["depth_scale"],
               dtype=torch.float32) -> torch.Tensor:
    """x (n, 90, 160) in ``dtype``: ``dagger.student_rows``' pixel rule.  One product per pixel."""
    return depth_pixels(image_buffer(depth).to(dtype), depth_clip, depth_scale)


class ConvStem(nn.Module):
    """The stem: x (n, 90, 160) -> features (n, 961), feature ``31 i + j`` = y(i, j).  torch's ``Conv2d`` default initialisation."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, CHANNELS, KERNEL, stride=STRIDE, padding=PADDING)
        self.conv2 = nn.Conv2d(CHANNELS, 1, 1)

    @classmethod
    def seeded(cls, seed: int) -> "ConvStem":
        """A stem initialised under ``seed``; the global generator is left as it was."""
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(int(seed))
            return cls()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 3 or tuple(x.shape[1:]) != (IMG_H, IMG_W):
            raise ValueError(f"the stem reads (n, {IMG_H}, {IMG_W}) images")
        y = self.conv2(F.leaky_relu(self.conv1(x.unsqueeze(1)), SLOPE))
        assert tuple(y.shape[1:]) == (1, SIDE, SIDE)
        return y.reshape(x.shape[0], FEATURES)

    def packed(self) -> torch.Tensor:
        """The 497 parameters as one vector: W1[8][6][10], b1[8], w2[8], b2."""
        return torch.cat([p.detach().reshape(-1) for p in (self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias)])

    @classmethod
    def from_packed(cls, vec: torch.Tensor, dtype=torch.float32) -> "ConvStem":
        m = cls().to(dtype)
        m.load_state_dict(unpack_stem(vec.to(dtype)))
        return m


def unpack_stem(vec: torch.Tensor) -> dict:
    """``ConvStem``'s state_dict (CPU tensors) from the packed 497 floats."""
    v = vec.detach().cpu().reshape(-1)
    if v.numel() != STEM_FLOATS:
        raise ValueError(f"the packed stem holds {STEM_FLOATS} floats")
    a, b, c = CHANNELS * TAPS, CHANNELS * TAPS + CHANNELS, CHANNELS * TAPS + 2 * CHANNELS
    return {"conv1.weight": v[:a].reshape(CHANNELS, 1, *KERNEL).clone(), "conv1.bias": v[a:b].clone(),
            "conv2.weight": v[b:c].reshape(1, CHANNELS, 1, 1).clone(), "conv2.bias": v[c:].clone()}


def conv_student_rows(stem: ConvStem, depth: torch.Tensor, env_rows: torch.Tensor, depth_clip: float = HPARAMS["depth_clip"],
                      depth_scale: float = HPARAMS["depth_scale"]) -> torch.Tensor:
    """The student rows (n, 965) in the dtype of ``env_rows``: the specification of ``rover_dagger_conv_rows``.  x is formed in float32
    (one product, as the kernel forms it) and widened."""
    x = preprocess(depth, depth_clip, depth_scale).to(env_rows.dtype)
    return torch.cat([sanitise(env_rows[:, :PROP]), stem(x)], dim=1)


def stem_backward(stem: ConvStem, x: torch.Tensor, g: torch.Tensor) -> dict:
    """The closed form the backward kernel evaluates: gradients of ``sum(g * stem(x))`` with respect to the four parameter blocks.
    ``x`` (n, 90, 160), ``g`` (n, 961).  The LeakyReLU's derivative at a pre-activation of exactly 0 is the slope."""
    n = x.shape[0]
    cols = F.unfold(x.unsqueeze(1), KERNEL, padding=PADDING, stride=STRIDE)               # (n, 60, 961); padded taps are 0
    w1 = stem.conv1.weight.detach().reshape(CHANNELS, TAPS)
    pre = torch.einsum("ct,nto->nco", w1, cols) + stem.conv1.bias.detach().view(1, CHANNELS, 1)
    h = torch.where(pre > 0, pre, pre * SLOPE)
    w2 = stem.conv2.weight.detach().reshape(CHANNELS)
    dpre = g.view(n, 1, FEATURES) * w2.view(1, CHANNELS, 1) * torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, SLOPE))
    return {"conv1.weight": torch.einsum("nco,nto->ct", dpre, cols).reshape(CHANNELS, 1, *KERNEL), "conv1.bias": dpre.sum((0, 2)),
            "conv2.weight": torch.einsum("no,nco->c", g, h).reshape(1, CHANNELS, 1, 1), "conv2.bias": g.sum().reshape(1)}


class ImageRing:
    """The preprocessed images beside a ``ReplayMemory(memory_size, num_envs)``: ``x`` is (memory_size + 1, num_envs, 14400) float32,
    one slot per slot of the memory's observation ring, addressed by the memory's own ring row number ``slot * num_envs + env``.  It
    has no counters of its own: the memory's cursor is the ring's."""

    def __init__(self, memory_size: int, num_envs: int, device="cuda"):
        if memory_size < 1 or num_envs < 1:
            raise ValueError("memory_size and num_envs must be >= 1")
        self.memory_size, self.num_envs, self.slots = int(memory_size), int(num_envs), int(memory_size) + 1
        self.device = torch.device(device)
        self.x = torch.zeros(self.slots, self.num_envs, PIXELS, dtype=torch.float32, device=self.device)

    @staticmethod
    def nbytes(memory_size: int, num_envs: int) -> int:
        return 4 * (int(memory_size) + 1) * int(num_envs) * PIXELS

    def fits(self, memory: ReplayMemory) -> bool:
        return self.slots >= memory.slots and self.num_envs == memory.num_envs and self.x.device == memory.obs.device

    def gather(self, memory: ReplayMemory, idx: torch.Tensor) -> torch.Tensor:
        """x (B, 90, 160) of the states of flat row indices, as ``memory.gather`` finds their rows."""
        idx = idx.to(self.device, torch.int64)
        k, e = idx // self.num_envs, idx % self.num_envs
        return self.x[memory.ring_pos[k].long(), e].view(-1, IMG_H, IMG_W)


def ring_counters(memory: ReplayMemory) -> dict:
    return {"memory_index": memory.memory_index, "filled": memory.filled, "cursor": memory.cursor}


def load_ring_counters(memory: ReplayMemory, sd: Mapping) -> None:
    memory.memory_index, memory.filled, memory.cursor = int(sd["memory_index"]), bool(sd["filled"]), int(sd["cursor"])
    memory._last_next, memory._last_version = None, -1


# ---------------------------------------------------------------------------------------------------------------- torch spec
class TorchConvDAgger:
    """One imitation step in torch autograd on stem and head together (``head``: ``Net(2, True)`` of examples/04_train_ppo.py); any
    dtype.  One Adam over both parameter lists, one ``clip_grad_norm_`` over both."""

    def __init__(self, head: nn.Module, stem: ConvStem, **hparams):
        self.hp = _hparams(hparams)
        self.student, self.stem = head, stem
        self._head_params = [p for k, p in head.named_parameters() if k != LOG_STD_KEY]
        self._stem_params = list(stem.parameters())
        self._params = self._head_params + self._stem_params
        self.optimizer = torch.optim.Adam(self._params, lr=self.hp["learning_rate"], betas=(self.hp["beta1"], self.hp["beta2"]),
                                          eps=self.hp["eps"])

    @property
    def dtype(self):
        return self._params[0].dtype

    def rows(self, env4: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        return torch.cat([env4, self.stem(x)], dim=1)

    def act(self, env_rows, depth):
        with torch.no_grad():
            return self.student(conv_student_rows(self.stem, depth, env_rows.to(self.dtype), self.hp["depth_clip"], self.hp["depth_scale"]))

    def step(self, env4: torch.Tensor, x: torch.Tensor, labels: torch.Tensor) -> dict:
        """One step on the rows' first four columns (B, 4), their images x (B, 90, 160) and labels (B, 2); returns loss, grad_norm
        (before clipping), dz, the rows with their recomputed features and dL/drow."""
        rows = self.rows(env4, x)
        rows.retain_grad()
        a = self.student(rows)
        loss = imitation_loss(a, labels)
        self.optimizer.zero_grad()
        loss.backward()
        norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in self._params]))
        if self.hp["grad_norm_clip"] > 0:
            nn.utils.clip_grad_norm_(self._params, self.hp["grad_norm_clip"])
        self.optimizer.step()
        return {"loss": float(loss.detach()), "grad_norm": float(norm), "dz": imitation_dz(a.detach(), labels),
                "rows": rows.detach(), "drow": rows.grad.detach().clone()}

    def update(self, memory: ReplayMemory, images: ImageRing, idx: torch.Tensor) -> dict:
        s, a, _, _, _ = memory.gather(idx)
        return self.step(s[:, :PROP].to(self.dtype), images.gather(memory, idx).to(self.dtype), a.to(self.dtype))

    def checkpoint(self) -> dict:
        return {"policy": {k: v.detach().clone() for k, v in self.student.state_dict().items()},
                STEM_KEY: {k: v.detach().clone() for k, v in self.stem.state_dict().items()}}


class _ConvCollectorBase(_DaggerCollectorBase):
    _image_buffer = staticmethod(image_buffer)

    def _ring(self, images: ImageRing) -> ImageRing:
        if not images.fits(self.memory):
            raise ValueError("the image ring must have the memory's envs, device and at least its slots")
        return images


class TorchConvDAggerCollector(TorchDAggerCollector, _ConvCollectorBase):
    """The specification, in torch / numpy: ``dagger.TorchDAggerCollector`` (its ``draws``, ``begin``, ``act`` and ``record``) with the
    stem in its rows.  ``teacher`` / ``student``: callables (n, 965) -> (n, 2) returning the tanh mean; ``stem``: a callable
    x (n, 90, 160) -> (n, 961)."""

    def __init__(self, teacher, student, stem, memory: ReplayMemory, images: ImageRing, seed: int = 42, env_id_offset: int = 0,
                 depth_clip: float = HPARAMS["depth_clip"], depth_scale: float = HPARAMS["depth_scale"]):
        super().__init__(teacher, student, memory, seed, env_id_offset, depth_clip, depth_scale)
        self.stem, self.images = stem, self._ring(images)

    def _rows(self, raw, depth, slot: int) -> None:
        x = preprocess(self._image(depth), self.depth_clip, self.depth_scale)
        self.images.x[slot] = x.reshape(self.n, PIXELS)
        self.memory.obs[slot] = torch.cat([sanitise(raw[:, :PROP]), self.stem(x).to(torch.float32)], dim=1)
        self.teacher_rows = sanitise(raw)

    @torch.no_grad()
    def resume(self, raw_obs) -> None:
        """What a resumed run calls in place of ``begin``: only the teacher's rows are refilled.  Both rings are the checkpoint's: the
        cursor slot keeps the features its last ``record`` wrote, one update older than the stem a ``begin`` would apply now."""
        self.teacher_rows = sanitise(self._raw(raw_obs))


# ---------------------------------------------------------------------------------------------------------------- fused
def fused_conv_rows(stem: torch.Tensor, depth: torch.Tensor, env_rows: torch.Tensor, out: torch.Tensor | None = None,
                    image_out: torch.Tensor | None = None, teacher_rows_out=None, depth_clip: float = HPARAMS["depth_clip"],
                    depth_scale: float = HPARAMS["depth_scale"], img_h: int = IMG_H, img_w: int = IMG_W) -> torch.Tensor:
    """One ``rover_dagger_conv_rows`` launch on the current stream: ``conv_student_rows`` on the device under the packed stem ``stem``
    (497 floats), with x into ``image_out`` (n, 14400) and optionally the sanitised env rows the teacher reads."""
    _fused.require_gpu("fused_conv_rows", "conv_student_rows is the CPU specification")
    d = image_buffer(depth)
    n, dev = int(env_rows.shape[0]), env_rows.device
    if out is None:
        out = torch.empty(n, OBS_DIM, dtype=torch.float32, device=dev)
    if image_out is None:
        image_out = torch.empty(n, PIXELS, dtype=torch.float32, device=dev)
    for name, t in (("stem", stem), ("depth", d), ("env_rows", env_rows), ("out", out), ("image_out", image_out),
                    ("teacher_rows_out", teacher_rows_out)):
        f32_cuda(name, t, dev, "the rows' device")
    holds("stem", stem, STEM_FLOATS)
    holds("depth", d, (n, PIXELS)); holds("image_out", image_out, (n, PIXELS))
    for name, t in (("env_rows", env_rows), ("out", out), ("teacher_rows_out", teacher_rows_out)):
        holds(name, t, (n, OBS_DIM))
    launch("rover_dagger_conv_rows", dev, C.byref(_collector_hparams(0, 0, depth_clip, depth_scale)), stem.data_ptr(), d.data_ptr(),
           int(img_h), int(img_w), env_rows.data_ptr(), n, out.data_ptr(), image_out.data_ptr(), ptr(teacher_rows_out), None, None, None,
           None, None, 0, None, 0, 0, C.c_uint64(0))
    return out


class FusedConvDAgger(FusedDAgger):
    """DAgger trainer state on the GPU for the 160 x 90 student: one vector ``[head | stem]`` (and Adam's moments in the same layout)
    and the device state struct (rover_dagger_state).  ``.actor`` aliases the head on replicas every update refreshes; ``.stem`` is
    the view of the stem's 497 floats that the collector's rows kernel reads, so the next ``record`` sees the new stem.  ``stem``:
    a ``ConvStem`` (or its state_dict); ``None`` initialises one with torch's ``Conv2d`` default under ``seed``."""

    _WORKSPACE, _PARAM_FLOATS = "rover_dagger_conv_workspace_bytes", "rover_dagger_conv_param_floats"
    _RUNS = "the reference policy network (Net(2, True)) behind the stem only (rover_dagger_conv.h)"

    def __init__(self, student_sd: Mapping[str, torch.Tensor], stem=None, device="cuda", n_copies: int = 4, seed: int = 42, **hparams):
        if stem is None:
            stem = ConvStem.seeded(seed)
        elif not isinstance(stem, nn.Module):
            m = ConvStem()
            m.load_state_dict(stem)
            stem = m
        self._stem0 = stem.packed().float().cpu().numpy()
        super().__init__(student_sd, device, n_copies, **hparams)

    def _flat(self, pa):
        """``[head | stem]``: the base's vector with the initial stem at ``stem_offset``."""
        self.stem_offset = int(self._lib.rover_dagger_conv_stem_offset(C.byref(self.desc_a)))
        self.chunk_rows = int(self._lib.rover_dagger_conv_chunk_rows())
        flat = super()._flat(pa)
        flat[self.stem_offset:self.stem_offset + STEM_FLOATS] = self._stem0
        del self._stem0                                            # from here on ``stem`` is the view of ``params``
        return flat

    @staticmethod
    def _checkpoint_args(ck):
        return ck["policy"], ck[STEM_KEY]

    # ---- views
    def stem_block(self, vec: torch.Tensor) -> torch.Tensor:
        return vec[self.stem_offset:self.stem_offset + STEM_FLOATS]

    @property
    def stem(self) -> torch.Tensor:
        """The stem's packed parameters: a view of ``params``."""
        return self.stem_block(self.params)

    def unstem(self, vec: torch.Tensor) -> dict:
        """``ConvStem``'s state_dict (float32 CPU) of the stem block of a vector in this layout."""
        return unpack_stem(self.stem_block(vec))

    def checkpoint(self) -> dict:
        """``{"policy": head state_dict, "student_stem": ConvStem state_dict}``: the head as ``FusedDAgger.checkpoint`` writes it."""
        ck = super().checkpoint()
        ck[STEM_KEY] = self.unstem(self.params)
        return ck

    def state_dict(self, memory: ReplayMemory | None = None) -> dict:
        """The checkpoint plus what a resumed run needs to continue bit for bit: the packed vectors, the device state and, with
        ``memory``, the ring's counters (the memory's and the image ring's contents are the caller's to keep)."""
        sd = super().state_dict()
        if memory is not None:
            sd["ring"] = ring_counters(memory)
        return sd

    def load_state_dict(self, sd: dict, memory: ReplayMemory | None = None) -> None:
        super().load_state_dict(sd)
        if memory is not None:
            load_ring_counters(memory, sd["ring"])

    # ---- kernels
    def update(self, memory: ReplayMemory, images: ImageRing, idx: torch.Tensor, dz_out: torch.Tensor | None = None,
               rows_out: torch.Tensor | None = None, drow_out: torch.Tensor | None = None, img_h: int = IMG_H, img_w: int = IMG_W) -> None:
        """One imitation step on rows ``idx`` of ``memory`` and their images (no host synchronisation).  ``rows_out`` / ``drow_out``
        (B, 965) receive the gathered rows with their recomputed features and dL/drow."""
        n = self._sample(memory, idx)
        if images.x.device != self.params.device or images.num_envs != memory.num_envs:
            raise ValueError("the image ring must have the memory's envs and device")
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rover_dagger_conv_update(
                C.byref(self.desc_a), C.byref(self.hp), self.params.data_ptr(), self.grad.data_ptr(), self.adam_m.data_ptr(),
                self.adam_v.data_ptr(), memory.obs.data_ptr(), images.x.data_ptr(), images.slots, int(img_h), int(img_w), memory.slots,
                memory.num_envs, memory.ring_pos.data_ptr(), memory.actions.data_ptr(), idx.data_ptr(), n, len(memory),
                self.ws.data_ptr(), self.ws.numel(), self.state.data_ptr(), self.rep_a.data_ptr(), self.n_copies,
                self._out(dz_out, 2 * n, "dz_out"), self._out(rows_out, OBS_DIM * n, "rows_out"),
                self._out(drow_out, OBS_DIM * n, "drow_out"), self._stream()), "rover_dagger_conv_update")


class ConvDAggerCollector(DAggerCollector, _ConvCollectorBase):
    """The fused collector of the 160 x 90 student.  ``act`` is ``DAggerCollector``'s, unchanged (two launches of
    ``rover_dagger_act``): the student's head reads the ring slot, whose feature columns ``begin`` / ``record`` filled.  ``begin`` and
    ``record`` are one launch each (``rover_dagger_conv_rows``): x into the image ring's slot, the stem's features under
    ``trainer.stem`` (held BY REFERENCE) into the ring slot, the record's bookkeeping."""

    def __init__(self, teacher, trainer: FusedConvDAgger, memory: ReplayMemory, images: ImageRing, seed: int = 42, env_id_offset: int = 0,
                 depth_clip: float = HPARAMS["depth_clip"], depth_scale: float = HPARAMS["depth_scale"]):
        super().__init__(teacher, trainer.actor, memory, seed, env_id_offset, depth_clip, depth_scale)
        self.trainer, self.images = trainer, self._ring(images)

    @torch.no_grad()
    def resume(self, raw_obs) -> None:
        """What a resumed run calls in place of ``begin``: only the teacher's rows are refilled (one torch ``nan_to_num``).  Both rings
        are the checkpoint's: the cursor slot keeps the features its last ``record`` wrote, one update older than the stem a ``begin``
        would apply now, so the run continues bit for bit."""
        self.teacher_rows.copy_(sanitise(self._raw(raw_obs)))

    def _record(self, raw, depth, ring_slot, counter=0, idx=None, rew=None, terminated=None, rew_out=None, term_out=None,
                ring_pos_entry=None, ring_pos_value=0, mem_rows=0) -> None:
        slot = ring_slot.storage_offset() // (self.n * OBS_DIM)            # the slot of the observation ring is the image ring's
        launch("rover_dagger_conv_rows", raw.device, C.byref(self.hparams()), self.trainer.stem.data_ptr(), self._image(depth).data_ptr(),
               IMG_H, IMG_W, raw.data_ptr(), self.n, ring_slot.data_ptr(), self.images.x[slot].data_ptr(), self.teacher_rows.data_ptr(),
               ptr(rew), ptr(terminated), ptr(rew_out), ptr(term_out), ptr(ring_pos_entry), int(ring_pos_value), ptr(idx),
               0 if idx is None else int(idx.numel()), int(mem_rows), C.c_uint64(int(counter)))


class ConvStudent:
    """The trained student for evaluation: ``act(env_rows, depth)`` -> (n, 2) from the env's raw rows and ``extras["depth"]`` of the
    160 x 90 camera: one rows launch and the head's inference kernel.  The returned buffer is overwritten by the next call."""

    def __init__(self, head, stem: torch.Tensor, depth_clip: float = HPARAMS["depth_clip"], depth_scale: float = HPARAMS["depth_scale"]):
        _fused.require_gpu("ConvStudent", "TorchConvDAgger.act is the CPU specification")
        self.head, self.stem = head, stem.detach().to(head.packed.device, torch.float32).contiguous()
        holds("stem", self.stem, STEM_FLOATS)
        self.depth_clip, self.depth_scale = float(depth_clip), float(depth_scale)
        self._rows = self._x = None

    @classmethod
    def from_checkpoint(cls, ck, **kw) -> "ConvStudent":
        from .policy import RoverNet
        ck = _fused.load_checkpoint(ck)
        stem = ConvStem()
        stem.load_state_dict(ck[STEM_KEY])
        return cls(RoverNet.from_state_dict(ck["policy"], final_act="tanh"), stem.packed(), **kw)

    @torch.no_grad()
    def act(self, env_rows: torch.Tensor, depth: torch.Tensor) -> torch.Tensor:
        if isinstance(env_rows, dict):
            env_rows = env_rows["policy"]
        n = int(env_rows.shape[0])
        if self._rows is None or self._rows.shape[0] != n:
            self._rows = torch.empty(n, OBS_DIM, dtype=torch.float32, device=env_rows.device)
            self._x = torch.empty(n, PIXELS, dtype=torch.float32, device=env_rows.device)
        fused_conv_rows(self.stem, depth, env_rows.contiguous(), out=self._rows, image_out=self._x, depth_clip=self.depth_clip,
                        depth_scale=self.depth_scale)
        return self.head(self._rows)
