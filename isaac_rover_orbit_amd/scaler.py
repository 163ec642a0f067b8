"""skrl's ``RunningStandardScaler`` on the MI355X at any width up to 1024 (C ABI: ``include/rover_scaler.h``).

``DeviceScaler`` holds one scaler block (float64 ``mean[w], var[w], count``) in device memory and runs the statistics update, the
forward and the inverse transform as HIP kernels: what the reference's agent files switch on with ``state_preprocessor`` /
``value_preprocessor`` (rover_envs/utils/config.py:76-96).  The torch specification is ``lift_ppo.RunningStandardScaler``; the
block layout is the lift trainer's.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping

import torch

from . import _fused, _lib


def default_hparams() -> "_lib.ScalerHparams":
    return _fused.default_hparams(_lib.ScalerHparams, "rover_scaler_default_hparams")


class DeviceScaler:
    """One ``RunningStandardScaler`` of ``width`` columns.  ``block`` is the device tensor the kernels read and write: whoever
    holds the scaler (a trainer and a rollout collector, say) sees every update at once."""

    def __init__(self, width: int, device="cuda", epsilon: float = 1e-8, clip_threshold: float = 5.0):
        _fused.require_gpu("DeviceScaler", "lift_ppo.RunningStandardScaler is the specification")
        self._lib = _lib.load()
        self.width = int(width)
        n = int(self._lib.rover_scaler_doubles(self.width))
        if n == 0:
            raise ValueError(f"width must be in [1, {_lib.SCALER_MAX_WIDTH}]")
        self.device = torch.device(device)
        self.hp = default_hparams()
        self.hp.eps, self.hp.clip = float(epsilon), float(clip_threshold)
        self.block = torch.zeros(n, dtype=torch.float64, device=self.device)    # mean 0, var 1, count 1
        self.block[self.width:] = 1.0
        self.device = self.block.device                                          # with its index
        self.ws = torch.empty(0, dtype=torch.uint8, device=self.device)

    # ---- views of the block
    @property
    def running_mean(self) -> torch.Tensor:
        return self.block[:self.width]

    @property
    def running_variance(self) -> torch.Tensor:
        return self.block[self.width:2 * self.width]

    @property
    def current_count(self) -> torch.Tensor:
        return self.block[2 * self.width]

    def state_dict(self) -> dict:
        """skrl's keys, float64 CPU tensors."""
        b, w = self.block.cpu(), self.width
        return {"running_mean": b[:w].clone(), "running_variance": b[w:2 * w].clone(), "current_count": b[2 * w].clone()}

    def load_state_dict(self, sd: Mapping[str, torch.Tensor]) -> None:
        w = self.width
        mean = torch.as_tensor(sd["running_mean"], dtype=torch.float64).reshape(-1)
        var = torch.as_tensor(sd["running_variance"], dtype=torch.float64).reshape(-1)
        if mean.numel() != w or var.numel() != w:
            raise ValueError(f"the checkpoint's scaler does not have {w} columns")
        self.block[:w] = mean.to(self.device)
        self.block[w:2 * w] = var.to(self.device)
        self.block[2 * w] = float(torch.as_tensor(sd["current_count"]))

    # ---- kernels
    def _stream(self):
        return _fused.stream(self.device)

    def _rows(self, x: torch.Tensor, name: str) -> torch.Tensor:
        if not x.is_cuda or x.dtype != torch.float32 or x.device != self.block.device:
            raise ValueError(f"{name} must be a float32 cuda tensor on the scaler's device")
        if x.numel() % self.width or not x.is_contiguous():
            raise ValueError(f"{name} must be contiguous rows of {self.width} columns")
        return x

    def _idx(self, idx):
        if idx is None:
            return None, None
        if not idx.is_cuda or idx.dtype != torch.int64 or not idx.is_contiguous() or idx.device != self.block.device:
            raise ValueError("idx must be a contiguous int64 cuda tensor on the scaler's device")
        return idx.data_ptr(), int(idx.numel())

    @torch.no_grad()
    def train(self, x: torch.Tensor, idx: torch.Tensor | None = None, gate: torch.Tensor | None = None) -> None:
        """Updates the statistics with the rows ``idx`` of ``x`` (all rows when ``idx`` is None); at least two rows.  ``gate``: an
        int32 device word (``FusedPPO.epoch_state[:1]``); the four launches return at once where it is not zero
        (``rover_scaler_train_gated``)."""
        x = self._rows(x, "x")
        ip, n = self._idx(idx)
        rows = x.numel() // self.width if n is None else n
        need = int(self._lib.rover_scaler_workspace_bytes(self.width, rows))
        if self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        if gate is not None:
            if not gate.is_cuda or gate.dtype != torch.int32 or gate.device != self.block.device or gate.numel() < 1:
                raise ValueError("gate must be an int32 cuda tensor on the scaler's device")
            _lib.check(self._lib.rover_scaler_train_gated(C.byref(self.hp), self.block.data_ptr(), self.width, x.data_ptr(), ip, rows,
                                                          self.ws.data_ptr(), self.ws.numel(), gate.data_ptr(), self._stream()),
                       "rover_scaler_train_gated")
            return
        _lib.check(self._lib.rover_scaler_train(C.byref(self.hp), self.block.data_ptr(), self.width, x.data_ptr(), ip, rows,
                                                self.ws.data_ptr(), self.ws.numel(), self._stream()), "rover_scaler_train")

    def _apply(self, x, idx, out, flags, raw_out):
        x = self._rows(x, "x")
        out = torch.empty_like(x) if out is None else self._rows(out, "out")
        ip, n = self._idx(idx)
        rows = x.numel() // self.width if n is None else n
        if n is None and out.numel() != x.numel():
            raise ValueError("out must have the shape of x")
        if raw_out is not None and (self._rows(raw_out, "raw_out").numel() != x.numel() and n is None):
            raise ValueError("raw_out must have the shape of x")
        _lib.check(self._lib.rover_scaler_apply(C.byref(self.hp), self.block.data_ptr(), self.width, x.data_ptr(), ip, rows, flags,
                                                out.data_ptr(), None if raw_out is None else raw_out.data_ptr(), self._stream()),
                   "rover_scaler_apply")
        return out

    @torch.no_grad()
    def forward(self, x: torch.Tensor, idx: torch.Tensor | None = None, out: torch.Tensor | None = None, sanitise: bool = False,
                raw_out: torch.Tensor | None = None) -> torch.Tensor:
        """``clamp((x - mean) / (sqrt(var) + eps), -clip, clip)``.  With ``idx`` only the rows it names are transformed, each into
        the same row of ``out`` (an image of ``x``'s shape; ``out`` is required then and its other rows are not touched).
        ``sanitise``: ``nan_to_num(nan=0, posinf=FLT_MAX, neginf=0)`` first, ``raw_out`` receives the sanitised rows."""
        if idx is not None and out is None:
            raise ValueError("with idx, out is the image the named rows are written into")
        return self._apply(x, idx, out, _lib.SCALER_SANITISE if sanitise else 0, raw_out)

    __call__ = forward

    @torch.no_grad()
    def inverse(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """``sqrt(var) * clamp(x, -clip, clip) + mean``."""
        return self._apply(x, None, out, _lib.SCALER_INVERSE, None)
