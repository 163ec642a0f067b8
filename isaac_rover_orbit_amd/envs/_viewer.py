"""What the envs with an rgb_array viewer share on the host: ``render()`` and its device-side forms, the
lazily created workspace and the rotating pair of frame buffers.  An env adds ``_viewer_native()`` (its config as the C struct),
``_viewer_bytes(vc)`` (the workspace size, raising its refusal when that is 0) and ``_viewer_render(vc, ws, rgba, dep, ids)``;
``_viewer_prepare(vc, ws, nb)`` runs once on a fresh workspace."""
from __future__ import annotations

import torch


def resolve_render_mode(render_mode, kwargs: dict):
    """``render_mode`` as the constructor honours it: the reference passes ``viewport=args_cli.video`` (train.py:123-125), which
    means ``"rgb_array"``.  Pops ``viewport`` from ``kwargs``."""
    if render_mode is None and kwargs.pop("viewport", False):
        render_mode = "rgb_array"
    return render_mode


class ViewerMixin:
    _viewer_ws = None

    def render(self):
        """``"rgb_array"``: the (H, W, 3) uint8 frame of the current state (a numpy view of a host copy, as ORBIT returns
        ``rgb_data[:, :, :3]``); otherwise None."""
        if self.render_mode != "rgb_array":
            return None
        return self.render_rgb().cpu().numpy()[:, :, :3]

    def _viewer_prepare(self, vc, ws, nb):
        pass

    def _viewer_workspace(self, vc):
        """The viewer's workspace, allocated (and prepared) on the first render."""
        if self._viewer_ws is None:
            with torch.cuda.device(self.device):
                nb = self._viewer_bytes(vc)
                ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=self.device)
                self._viewer_prepare(vc, ws, nb)
            self._viewer_ws, self._viewer_ws_bytes = ws, nb
            self._viewer_buf = []
            self._viewer_cur = 0
        return self._viewer_ws

    def render_frame(self, depth: bool = False, object_id: bool = False):
        """A fresh viewer frame of the current state in new device buffers: (rgba (H, W, 4) uint8, depth (H, W) fp32 or None,
        object_id (H, W) int32 or None), asynchronous on the current stream."""
        vc = self._viewer_native()
        ws = self._viewer_workspace(vc)
        h, w = vc.height, vc.width
        rgba = torch.empty(h, w, 4, dtype=torch.uint8, device=self.device)
        dep = torch.empty(h, w, dtype=torch.float32, device=self.device) if depth else None
        ids = torch.empty(h, w, dtype=torch.int32, device=self.device) if object_id else None
        self._viewer_render(vc, ws, rgba, dep, ids)
        return rgba, dep, ids

    def render_rgb(self) -> torch.Tensor:
        """The viewer frame of the current state as a device (H, W, 4) uint8 RGBA tensor, without a host synchronisation.  Two
        buffers rotate, so the frame one call returns stays valid through the next call."""
        vc = self._viewer_native()
        ws = self._viewer_workspace(vc)
        shape = (vc.height, vc.width, 4)
        if not self._viewer_buf or tuple(self._viewer_buf[0].shape) != shape:
            self._viewer_buf = [torch.empty(shape, dtype=torch.uint8, device=self.device) for _ in range(2)]
        self._viewer_cur ^= 1
        buf = self._viewer_buf[self._viewer_cur]
        self._viewer_render(vc, ws, buf)
        return buf
