"""``SensorRig``: the rover env's depth camera (render -> sensor model -> noise / clip), lidar (cast -> noise / clip) and the rolling
elevation map one of them feeds, with the schedule that runs them behind a step.  The schedule reaches the
stages only through ``render``, ``.apply``, ``.cast``, ``.update`` and ``.clear``, so it runs on the CPU over stand-ins."""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib
from .._fused import launch, stream
from ..depth_sensor import DepthSensor
from ..elevation import ElevationMap
from ..lidar import Lidar, elevation_geometry
from ..obs_post import DEPTH_TAG, LIDAR_TAG, ObsPost, image_segments, lidar_segments

KEYS = ("depth", "depth_valid", "rgb", "lidar_range", "lidar_hits_w", "elevation_scan", "elevation_known", "elevation_count")
FILL_KEYS = ("elevation_scan_filled", "elevation_fill_dist", "elevation_filled_count")      # only under ElevationMapCfg.fill
TRAVERSE_KEYS = ("elevation_cost", "elevation_cost_class", "elevation_lethal_count")        # only under ElevationMapCfg.traverse


class Rotating:
    """``nbuf`` sets of buffers that rotate like the env's observation buffers: what ``next()`` hands out stays untouched through
    the ``next()`` after it.  ``next()`` publishes the set in ``extras`` under ``keys`` (or those it is given) but for a ``None``."""

    def __init__(self, extras: dict, keys, make, nbuf: int = 2):
        self.extras, self.keys, self.sets, self.cur = extras, keys, [make() for _ in range(nbuf)], -1
        self.next()

    def next(self, keys=None):
        self.cur = (self.cur + 1) % len(self.sets)
        self.extras.update((k, t) for k, t in zip(keys or self.keys, self.sets[self.cur]) if t is not None)
        return self.sets[self.cur]


class SensorRig:
    """``host`` (the env) has ``extras``, ``common_step_counter`` and ``call_counter``; ``for_env`` builds the device parts, which
    are plain attributes: a bench switches a stage off by setting it to ``None``.  ``render(camera_cfg, workspace, buf)`` fills the
    (N, H, W) ``buf``; ``image``: (H, W); ``pose``: the (pos, quat) views the map reads; ``map_source``: "camera" or "lidar"; ``fill_iterations``: 0, or the sweeps
    of the min-fill launch that follows every map launch (``elevation.fill``) into buffers of its own; ``traverse``: ``None``, or the
    ``TraverseCfg`` of the launch behind the two (``elevation.traverse``), which reads the fill's window where there is a fill and
    the map where there is none, and writes into buffers of its own."""

    def __init__(self, host, device="cpu", num_envs: int = 0, nbuf: int = 2, render=None, camera_cfg=None, workspace=None, image=None,
                 depth_sensor=None, depth_post=None, camera_every: int = 1, lidar=None, lidar_post=None, lidar_hits: bool = False,
                 lidar_every: int = 1, elevation=None, map_source: str = "camera", unknown_value: float = 0.0, pose=None, fill_iterations: int = 0,
                 traverse=None):
        self.host, self._render, self.camera_cfg, self.workspace = host, render, camera_cfg, workspace
        self.depth_sensor, self.depth_post, self.camera_every = depth_sensor, depth_post, int(camera_every)
        self.lidar, self.lidar_post, self.lidar_every = lidar, lidar_post, int(lidar_every)
        self.elevation, self.map_source, self._pose = elevation, map_source, pose
        self.fill_iterations = int(fill_iterations) if elevation is not None else 0
        self.traverse = traverse if elevation is not None else None
        self.active = camera_cfg is not None or lidar is not None
        ex, n, inf = host.extras, int(num_envs), float("inf")
        for key in KEYS + FILL_KEYS + TRAVERSE_KEYS:                       # what the rig before this one published
            ex.pop(key, None)
        full = lambda shape, value, dtype=torch.float32: torch.full(shape, value, dtype=dtype, device=device)      # noqa: E731
        if camera_cfg is not None:       # extras["depth"]: the (N, W, H) view of the row-major (N, H, W) image the kernels write
            self._depth = Rotating(ex, KEYS[:2], lambda: (full((n, *image), inf).permute(0, 2, 1),
                                                          None if depth_sensor is None else full((n,), 0, torch.int32)), nbuf)
            ex["rgb"] = None             # what the reference's listener reports without RGB data (rover_camera_env.py:94-98)
        if lidar is not None:
            self._ranges = Rotating(ex, KEYS[3:5], lambda: (full((n, lidar.channels, lidar.azimuths), inf),
                                                            full((n, lidar.rays, 3), inf) if lidar_hits else None), nbuf)
        if elevation is not None:
            self._maps = Rotating(ex, KEYS[5:], lambda: (full((n, elevation.columns), float(unknown_value)),
                                                         full((n, elevation.columns), 0, torch.uint8), full((n,), 0, torch.int32)), nbuf)
            self._mask = full((n,), 0, torch.uint8)                        # the envs of a partial reset
        if self.fill_iterations:
            self._fills = Rotating(ex, FILL_KEYS, lambda: (full((n, elevation.columns), float(unknown_value)),
                                                           full((n, elevation.columns), 255, torch.uint8), full((n,), 0, torch.int32)), nbuf)
        if self.traverse is not None:
            self._costs = Rotating(ex, TRAVERSE_KEYS, lambda: (full((n, elevation.columns), float(self.traverse.unknown_cost)),
                                                               full((n, elevation.columns), 0, torch.uint8), full((n,), 0, torch.int32)), nbuf)
            # the fill's window, handed on to the traverse launch on the same stream: one buffer is enough
            self._filled = full((n, elevation.grid, elevation.grid), float("nan")) if self.fill_iterations else None

    @classmethod
    def for_env(cls, env) -> "SensorRig":
        """The rig of ``env.cfg`` on ``env``'s handle.  The camera's workspace (the terrain's max-height pyramid) is built here and
        the lidar adopts it; a lidar without a camera prepares its own: one pyramid either way."""
        cfg, n, dev = env.cfg, env.num_envs, env.device
        cam, lid, emc = cfg.camera, getattr(cfg, "lidar", None), cfg.elevation
        keyed = {"seed": int(cfg.seed), "env_id_offset": int(cfg.env_id_offset)}
        kw = {"pose": (env.state[_lib.POS:_lib.POS + 3].t(), env.state[_lib.QUAT:_lib.QUAT + 4].t())}
        if emc is not None:
            kw.update(map_source=getattr(emc, "source", "camera"), unknown_value=emc.unknown_value,
                      fill_iterations=emc.fill_iterations if getattr(emc, "fill", "none") != "none" else 0,
                      traverse=getattr(emc, "traverse", None))
        if cam is not None:
            native, noisy = cam.to_native(), cam.noise is not None or cam.clip is not None
            kw.update(camera_cfg=native, image=(int(cam.height), int(cam.width)), camera_every=cam.every_n_steps,
                      depth_sensor=DepthSensor.from_camera(cam, **keyed) if cam.sensor is not None else None,
                      depth_post=ObsPost(image_segments(cam), int(cam.height) * int(cam.width), tag=DEPTH_TAG, **keyed) if noisy else None)
            nb = int(env._lib.rover_camera_workspace_bytes(env._h, C.byref(native)))
            if nb == 0:
                raise _lib.RoverHipError("rover_camera_workspace_bytes: no terrain bound or invalid camera config")
            kw["workspace"] = ws = torch.zeros((nb + 3) // 4, dtype=torch.float32, device=dev)
            launch("rover_camera_prepare", dev, env._h, C.byref(native), ws.data_ptr(), nb)
            kw["render"] = lambda native, ws, buf: _lib.check(env._lib.rover_camera_render(
                env._h, C.byref(native), ws.data_ptr(), buf.data_ptr(), stream(dev)), "rover_camera_render")
            if kw.get("map_source") == "camera":                           # the map: one launch behind the camera chain
                kw["elevation"] = ElevationMap(emc, cam, cfg.height_scanner, n, dev)
        if lid is not None:
            L = Lidar(lid, env, workspace=kw.get("workspace"))
            if L.workspace is None:
                L.prepare()
            noisy = lid.noise is not None or lid.clip is not None
            kw.update(lidar=L, lidar_hits=bool(lid.hits), lidar_every=lid.every_n_steps,
                      lidar_post=ObsPost(lidar_segments(lid), L.rays, tag=LIDAR_TAG, **keyed) if noisy else None)
            if kw.get("map_source") == "lidar":                            # the map: behind the lidar chain, fed the lidar's own table
                kw["elevation"] = ElevationMap(emc, elevation_geometry(lid), cfg.height_scanner, n, dev, rays=L._rays32)
        return cls(env, dev, n, env._nbuf, **kw)

    def _counter(self) -> int:
        """The call counter the last reset() / step() launch ran under: it keys the draws of every frame of the state it left."""
        return max(self.host.call_counter - 1, 0)

    def render_into(self, buf: torch.Tensor, valid: torch.Tensor | None = None):
        """The depth image of the current state into the row-major (N, H, W) ``buf``, then the sensor model (its per-env count of
        valid pixels into ``valid``), then noise and clip, all in place; a re-render of the same state repeats its noise."""
        self._render(self.camera_cfg, self.workspace, buf)
        if self.depth_sensor is not None:
            self.depth_sensor.apply(buf, self._counter(), valid_out=valid)
        if self.depth_post is not None:
            self.depth_post.apply(buf, self._counter())

    def cast_into(self, buf: torch.Tensor, hits: torch.Tensor | None = None):
        """The lidar frame of the current state into the (N, channels, azimuths) ``buf``, then noise and clip in place."""
        self.lidar.cast(buf, hits)
        if self.lidar_post is not None:
            self.lidar_post.apply(buf, self._counter())

    def render_depth(self) -> torch.Tensor:
        if self.camera_cfg is None:
            raise RuntimeError("render_depth needs a camera (cfg.camera)")
        buf = torch.empty_like(self._depth.sets[0][0].permute(0, 2, 1))
        self.render_into(buf)
        return buf.permute(0, 2, 1)

    def cast_lidar(self) -> torch.Tensor:
        if self.lidar is None:
            raise RuntimeError("cast_lidar needs a lidar (cfg.lidar)")
        buf = torch.empty_like(self._ranges.sets[0][0])
        self.cast_into(buf)
        return buf

    def _map_update(self, frame, reset):
        """One map launch into the next set of outputs; ``frame`` None: scroll and scan only."""
        scan, known, count = self._maps.next()
        self.elevation.update(frame, *self._pose, reset=reset, scan_out=scan, known_out=known, count_out=count)
        if self.fill_iterations:                                           # the same pose, the map the launch above left
            scan, dist, count = self._fills.next()
            window = {} if self.traverse is None else {"filled_out": self._filled}
            self.elevation.fill(*self._pose, scan_out=scan, dist_out=dist, count_out=count, iterations=self.fill_iterations, **window)
        if self.traverse is not None:                                      # the fill's window, or the map itself
            scan, cls, count = self._costs.next()
            self.elevation.traverse(*self._pose, heights=self._filled, scan_out=scan, class_out=cls, count_out=count, cfg=self.traverse)

    def _lidar_update(self, force: bool, reset):
        buf = None
        if force or self.host.common_step_counter % self.lidar_every == 0:
            buf, hits = self._ranges.next()
            self.cast_into(buf, hits)
        if self.elevation is not None and self.map_source == "lidar":
            self._map_update(buf, reset)

    def update(self, force: bool = False, reset=(None, None)):
        """Frames of the pose the step (or reset) left behind, each sensor on its own ``every_n_steps`` (``force``: both), the lidar
        first.  The map is updated on every call, with ``None`` where its sensor made no frame; the envs of ``reset`` start over."""
        if self.lidar is not None:
            self._lidar_update(force, reset)
        if self.camera_cfg is None:
            return
        buf = None
        if force or self.host.common_step_counter % self.camera_every == 0:
            view, valid = self._depth.next(KEYS[:2] if self.depth_sensor is not None else KEYS[:1])   # counts: under a sensor model only
            buf = view.permute(0, 2, 1)
            self.render_into(buf, valid)
        if self.elevation is not None and self.map_source == "camera":
            self._map_update(buf, reset)

    def update_after_draws(self, mask=None):
        """Behind ``reset_with_draws``: the masked envs' (``None``: all) maps start over with a frame of their new pose.  Without a
        map the lidar alone takes a frame, and a camera alone takes none: ``extras["depth"]`` keeps the previous frame."""
        if self.elevation is not None:
            self._mask.fill_(1) if mask is None else self._mask.copy_(mask)
            self.update(force=True, reset=(self._mask, None))
        elif self.lidar is not None:
            self._lidar_update(True, (None, None))

    def clear(self):
        if self.elevation is not None:
            self.elevation.clear()

    def reseed(self, seed: int):
        for stage in (self.depth_sensor, self.depth_post, self.lidar_post):
            if stage is not None:
                stage.seed = seed

    def state_dict(self) -> dict:
        return {} if self.elevation is None else self.elevation.state_dict()

    def load_state_dict(self, sd: dict):
        if self.elevation is not None and "elevation_map" in sd:
            self.elevation.load_state_dict(sd)
