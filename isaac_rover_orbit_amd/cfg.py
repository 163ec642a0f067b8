"""Declarative configuration of ``AAURoverEnv-v0`` in the *shape* of the reference's ORBIT ``@configclass`` tables
(term name -> func / weight / params), so that user cfg edits carry over:

* ``RoverEnvCfg``          <- ``rover_envs/envs/navigation/rover_env_cfg.py:228-278``
* ``AckermannActionCfg``   <- ``rover_envs/mdp/actions/actions_cfg.py:9-51``
* ``AAURoverEnvCfg``       <- ``rover_envs/envs/navigation/robots/aau_rover/env_cfg.py:10-31``

The built-in term *functions* are fused into the HIP kernels; the cfg carries their names (strings), weights, scales and
thresholds, which are compiled into the kernel parameter block (``_lib.RoverConfig``).

**User-written terms** (the normal way to use the reference: ``rover_env_cfg.py:126-183`` are tables of arbitrary ``func=``):
a reward or termination entry whose ``func`` is a *callable* -- signature ``func(env, **params) -> (num_envs,) tensor``, as in
``mdp/rewards.py:14-137`` / ``mdp/terminations.py:14-64`` -- is kept and evaluated in torch by ``RoverEnv.step`` on the env's
manager / scene facades between the two halves of the step (``rover_step_begin`` / ``rover_step_finish``: the SLOW path, three
launches + the torch ops of the terms).  The built-in entries must stay in the table (a built-in reward is switched off with
``weight=0``); with the stock table the env takes the one-launch fast path.  The observation TERMS are fixed (they define the row
layout the policy checkpoint expects); their ORBIT post-processing -- ``noise`` (``Unoise(n_min, n_max)``, imported for that by
``rover_env_cfg.py:23``), ``clip``, and a ``scale`` on the terms the kernels do not scale -- is applied in torch on the finished
row, in ORBIT's order (noise, clip, scale), for the terms that ask for it (``RoverEnvCfg.observation_post``).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Any

from . import _lib


@dataclass
class TermCfg:
    func: Any            # the name of a built-in term function (str) or a user callable func(env, **params)
    weight: float = 1.0
    scale: float = 1.0
    params: dict = field(default_factory=dict)
    time_out: bool = False
    noise: Any = None    # observation terms: ORBIT NoiseCfg (``noise.func(data, noise)``) or an object with n_min / n_max, mean / std, bias
    clip: Any = None     # observation terms: (min, max)


@dataclass
class SceneCfg:
    num_envs: int = 256          # rover_env_cfg.py:233-234
    env_spacing: float = 4.0
    replicate_physics: bool = False


@dataclass
class SimCfg:
    dt: float = 1.0 / 30.0       # rover_env_cfg.py:269
    device: str = "cuda:0"
    use_gpu_pipeline: bool = True


@dataclass
class RayCasterCfg:
    """``height_scanner`` (rover_env_cfg.py:78-86)."""
    resolution: float = 0.1
    size: tuple = (3.0, 3.0)
    offset_z: float = 10.0
    attach_yaw_only: bool = True
    max_distance: float = 100.0
    height_offset: float = 0.26878   # observations.py:45
    # what the vertical rays hit: "triangles" = the triangle mesh of the heightfield (each cell split along its
    # (i, j) - (i+1, j+1) diagonal; what ORBIT's Warp mesh ray-cast of that terrain returns), "bilinear" = smooth patch
    surface: str = "triangles"

    @property
    def grid(self):
        # ORBIT patterns.grid_pattern: arange(-size/2, size/2 + 1e-9, resolution)
        nx = int(math.floor((self.size[0] + 1e-9) / self.resolution)) + 1
        ny = int(math.floor((self.size[1] + 1e-9) / self.resolution)) + 1
        return nx, ny


@dataclass
class AckermannActionCfg:
    """actions_cfg.py:9-51 with the AAU values of aau_rover/env_cfg.py:21-31."""
    asset_name: str = "robot"
    scale: tuple = (1.0, 1.0)
    offset: Any = -0.0135            # scalar => broadcast to both channels (reference quirk B-4)
    wheelbase_length: float = 0.849
    middle_wheel_distance: float = 0.894
    rear_and_front_wheel_distance: float = 0.77
    wheel_radius: float = 0.1
    min_steering_radius: float = 0.8
    steering_joint_names: tuple = (".*Steer_Revolute",)
    drive_joint_names: tuple = (".*Drive_Continuous",)


@dataclass
class CommandCfg:
    """CommandsCfg.target_pose (rover_env_cfg.py:187-200) + RoverTerrainImporter.target_distance (terrain_importer.py:132)."""
    resampling_time_range: tuple = (150.0, 150.0)
    heading_range: tuple = (-math.pi, math.pi)
    simple_heading: bool = False
    target_distance: float = 9.0
    max_target_tries: int = 32


@dataclass
class TerrainCfg:
    """Synthetic stand-in for the missing terrain USDs: ``kind`` in {"procedural", "flat", "custom"}."""
    kind: str = "procedural"
    shape: tuple = (2048, 2048)
    seed: int = 1234
    sigma_z: float = 0.15
    n_rocks: int = 400
    terrain: Any = None              # an isaac_rover_orbit_amd.terrain.Terrain for kind == "custom"
    spawn_seed: int = 41


@dataclass
class DepthSensorCfg:
    """A stereo / structured-light depth sensor in front of the rendered depth (include/rover_depth_sensor.h, depth_sensor.py):
    a working range, pixel dropout that is likelier on depth edges, axial noise sigma(z) = sigma[0] + sigma[1] z + sigma[2] z^2
    and disparity quantisation, in that order; a pixel without data reads ``invalid_value``.  The defaults change nothing but a
    miss (+inf stays valid under ``range_max = inf``)."""
    range_min: float = 0.0                             # m
    range_max: float = math.inf
    sigma: tuple = (0.0, 0.0, 0.0)                     # m, 1, 1 / m
    p_drop: float = 0.0                                # dropout probability of a pixel off an edge
    p_edge: float = 0.0                                # ... of a pixel on one
    edge_rel: float = 0.1                              # |z - zn| > edge_rel * min(z, zn) to a 4-neighbour makes an edge
    edge_at_invalid: bool = True                       # a neighbour outside the range makes one too
    disparity_step: float = 0.0                        # px; 0 = no quantisation
    baseline: float = 0.05                             # m
    invalid_value: float = 0.0                         # what depth cameras report

    def to_native(self, focal_px: float) -> "_lib.DepthSensorCfg":
        """The library's struct, checked as the library checks it (the values as the fp32 struct holds them); ``focal_px`` is the
        camera's horizontal focal length in pixels: fb = float32(focal_px * baseline) and inv_step = float32(1 / step), both
        formed in double."""
        if len(tuple(self.sigma)) != 3:
            raise ValueError("depth sensor sigma must be (sigma0, sigma1, sigma2)")
        c = _lib.DepthSensorCfg()
        c.range_min, c.range_max = float(self.range_min), float(self.range_max)
        c.sigma0, c.sigma1, c.sigma2 = (float(v) for v in self.sigma)
        c.p_drop, c.p_edge, c.edge_rel = float(self.p_drop), float(self.p_edge), float(self.edge_rel)
        c.edge_at_invalid = 1 if self.edge_at_invalid else 0
        c.disparity_step, c.invalid_value = float(self.disparity_step), float(self.invalid_value)
        ok = lambda v: math.isfinite(v) and v >= 0.0   # noqa: E731
        if not (ok(c.sigma0) and ok(c.sigma1) and ok(c.sigma2) and ok(c.edge_rel)):
            raise ValueError("depth sensor sigma and edge_rel must be finite and >= 0")
        if not (0.0 <= c.p_drop <= 1.0 and 0.0 <= c.p_edge <= 1.0):
            raise ValueError("depth sensor p_drop and p_edge must be in [0, 1]")
        if not c.range_min >= 0.0 or not c.range_max >= c.range_min:
            raise ValueError("depth sensor range must satisfy 0 <= range_min <= range_max (range_max may be inf)")
        if not ok(c.disparity_step):
            raise ValueError("depth sensor disparity_step must be finite and >= 0")
        if c.disparity_step > 0.0:
            c.fb = float(focal_px) * float(self.baseline)
            c.inv_step = 1.0 / float(self.disparity_step)
            if not (math.isfinite(c.fb) and c.fb > 0.0 and math.isfinite(c.inv_step) and c.inv_step > 0.0):
                raise ValueError("depth sensor focal length * baseline and 1 / disparity_step must be finite and > 0")
        if math.isnan(c.invalid_value):
            raise ValueError("depth sensor invalid_value must not be a NaN")
        return c


@dataclass
class TraverseCfg:
    """Slope, step height, roughness and a traversability cost from the elevation map (include/rover_elevation_traverse.h): per
    cell over its (2 ``radius`` + 1)^2 neighbourhood.  A cell is lethal when one of the three reaches its ``*_crit``; otherwise its
    cost is the weighted sum of the three ratios.  The defaults are the implementer's choice, not tuned values."""
    radius: int = 2                                    # cells, in [1, 4]
    min_support: int = 1                               # usable cells (centre included) a cell needs, in [1, (2 radius + 1)^2]
    slope_crit: float = 0.577                          # a tangent: tan 30 deg
    step_crit: float = 0.3                             # m
    rough_crit: float = 0.1                            # m
    w_slope: float = 0.4
    w_step: float = 0.4
    w_rough: float = 0.2
    unknown_cost: float = 1.0                          # what a scan column without a cost reads

    def check(self):
        """ValueError for what the library refuses, on the values as the fp32 struct holds them."""
        f32 = lambda x: C.c_float(float(x)).value      # noqa: E731
        for name in ("radius", "min_support"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"traverse {name} must be an integer")
        if not 1 <= self.radius <= _lib.ELEVATION_TRAVERSE_MAX_RADIUS:
            raise ValueError(f"traverse radius must be in [1, {_lib.ELEVATION_TRAVERSE_MAX_RADIUS}]")
        if not 1 <= self.min_support <= (2 * self.radius + 1) ** 2:
            raise ValueError("traverse min_support must be in [1, (2 radius + 1)^2]")
        for name in ("slope_crit", "step_crit", "rough_crit"):
            v = f32(getattr(self, name))
            if not (math.isfinite(v) and v > 0.0):
                raise ValueError(f"traverse {name} must be finite and > 0")
        w = [f32(getattr(self, name)) for name in ("w_slope", "w_step", "w_rough")]
        if not all(math.isfinite(v) and v >= 0.0 for v in w):
            raise ValueError("traverse weights must be finite and >= 0")
        if not f32(f32(w[0] + w[1]) + w[2]) <= 1.0:
            raise ValueError("traverse weights must sum to at most 1 (in fp32, (w_slope + w_step) + w_rough)")
        if math.isnan(f32(self.unknown_cost)):
            raise ValueError("traverse unknown_cost must not be a NaN")

    def to_native(self) -> "_lib.ElevationTraverseCfg":
        self.check()
        return _lib.ElevationTraverseCfg(int(self.radius), int(self.min_support), float(self.slope_crit), float(self.step_crit),
                                         float(self.rough_crit), float(self.w_slope), float(self.w_step), float(self.w_rough),
                                         float(self.unknown_cost))


@dataclass
class ElevationMapCfg:
    """A rolling, robot-centric elevation map built from the depth camera (include/rover_elevation.h, elevation.py): ``grid`` x
    ``grid`` world-anchored cells of ``cell`` metres around the rover, fed by the pixels within ``[range_min, range_max]``, the
    cell's height the frame's maximum, blended into a known cell with weight ``alpha``.  The policy's height scan is read out of
    the map; a column over an unknown cell reads ``unknown_value``."""
    cell: float = 0.1                                  # m
    grid: int = 64                                     # cells per side: a power of two in [8, 128]
    range_min: float = 0.1                             # m, > 0: the depth sensor's invalid_value = 0 falls out here
    range_max: float = 5.0
    alpha: float = 1.0                                 # 1 = the newest frame replaces a cell's height
    unknown_value: float = 0.0
    # which sensor feeds the map: "camera" (cfg.camera's depth image) or "lidar" (cfg.lidar's range frame; full attitude only)
    source: str = "camera"
    # inpainting behind every map update (include/rover_elevation_fill.h): "none", or "min" -- unknown cells take the minimum of
    # their known neighbours, ring by ring, at most ``fill_iterations`` cells far; published next to the raw scan, never in its place
    fill: str = "none"
    fill_iterations: int = 32
    # slope / step / roughness / cost layers behind every map update, after the fill if there is one (TraverseCfg); None: no launch
    traverse: TraverseCfg | None = None

    def check(self):
        """ValueError for what the library refuses, on the values as the fp32 struct holds them."""
        f32 = lambda x: C.c_float(float(x)).value      # noqa: E731
        if self.traverse is not None:
            self.traverse.check()
        if self.source not in ("camera", "lidar"):
            raise ValueError("elevation source must be 'camera' or 'lidar'")
        if self.fill not in ("none", "min"):
            raise ValueError("elevation fill must be 'none' or 'min'")
        it = self.fill_iterations
        if isinstance(it, bool) or not isinstance(it, int) or not 1 <= it <= _lib.ELEVATION_FILL_MAX_ITERATIONS:
            raise ValueError(f"elevation fill_iterations must be an integer in [1, {_lib.ELEVATION_FILL_MAX_ITERATIONS}]")
        g = int(self.grid)
        if g != self.grid or g < _lib.ELEVATION_MIN_GRID or g > _lib.ELEVATION_MAX_GRID or g & (g - 1):
            raise ValueError(f"elevation grid must be a power of two in [{_lib.ELEVATION_MIN_GRID}, {_lib.ELEVATION_MAX_GRID}]")
        cell = f32(self.cell)
        inv_cell = f32(1.0 / float(self.cell)) if math.isfinite(cell) and cell > 0.0 else math.nan
        if not (math.isfinite(inv_cell) and inv_cell > 0.0):
            raise ValueError("elevation cell and 1 / cell must be finite and > 0")
        lo, hi = f32(self.range_min), f32(self.range_max)
        if not (math.isfinite(lo) and lo > 0.0 and hi >= lo):
            raise ValueError("elevation range must satisfy 0 < range_min <= range_max (range_max may be inf)")
        if not 0.0 < f32(self.alpha) <= 1.0:
            raise ValueError("elevation alpha must be in (0, 1]")
        if math.isnan(f32(self.unknown_value)):
            raise ValueError("elevation unknown_value must not be a NaN")

    def to_native(self, mount_pos, height_offset: float) -> "_lib.ElevationCfg":
        """The library's struct: ``mount_pos`` is the camera's position on the Body link, ``height_offset`` the height scanner's;
        inv_cell = float32(1 / cell), formed in double."""
        self.check()
        c = _lib.ElevationCfg()
        c.cell, c.inv_cell, c.grid = float(self.cell), 1.0 / float(self.cell), int(self.grid)
        c.range_min, c.range_max, c.alpha = float(self.range_min), float(self.range_max), float(self.alpha)
        if len(tuple(mount_pos)) != 3 or not all(math.isfinite(C.c_float(float(v)).value) for v in mount_pos):
            raise ValueError("elevation mount_pos must be three finite values")
        for i in range(3):
            c.mount_pos[i] = float(mount_pos[i])
        c.height_offset, c.unknown_value = float(height_offset), float(self.unknown_value)
        if math.isnan(c.height_offset):
            raise ValueError("elevation height_offset must not be a NaN")
        return c


@dataclass
class CameraCfg:
    """The rover's on-board depth camera (``RoverEnvCamera``, rover_camera_env.py:44-62): a pinhole on the Body link whose
    ``distance_to_camera`` image is a ray cast against the terrain's triangle mesh (include/rover_camera.h; RGB is not rendered)."""
    width: int = 160                                   # render product (:62)
    height: int = 90
    focal_length: float = 2.12                         # mm (:47)
    horizontal_aperture: float = 6.055                 # mm (:49): f = 160 * 2.12 / 6.055 = 56.02 px, horizontal FOV 110.0 deg
    # None = square pixels (Isaac Sim derives the vertical extent from the aspect ratio: vertical FOV 77.5 deg); the stated
    # verticalAperture of :50 is 2.968879962 (vertical FOV 70.0 deg)
    vertical_aperture: float | None = None
    position: tuple = (-0.151, 0.0, 0.73428)           # m, Body frame (:55)
    orientation: tuple = (0.64086, 0.29884, -0.29884, -0.64086)   # (w, x, y, z), USD camera convention (:56); normalised
    near_clip: float = 0.01                            # m (:51 clippingRange)
    far_clip: float = 1000000.0
    every_n_steps: int = 1                             # re-render on steps with common_step_counter % every_n_steps == 0
    # sensor noise on the rendered image, then a clip (obs_post.py: one HIP launch behind the render, draws keyed by the seed, the
    # global env id, the call counter and the pixel); both None = the image as rendered, nothing launched.  Misses stay +inf unless
    # a clip brings them to its upper bound.
    noise: Any = None                                  # an object with n_min / n_max, mean / std or bias
    clip: Any = None                                   # (min, max), finite
    # a depth sensor model between the render and noise / clip (depth_sensor.py: one HIP launch of its own, keyed the same way);
    # None = nothing launched.  With one, extras["depth_valid"] counts each env's pixels that carry data.
    sensor: DepthSensorCfg | None = None

    @property
    def focal_px(self) -> tuple:
        """(f_x, f_y) in pixels."""
        fx = self.width * self.focal_length / self.horizontal_aperture
        fy = fx if self.vertical_aperture is None else self.height * self.focal_length / self.vertical_aperture
        return fx, fy

    def validate(self):
        """The checks of the library's config_ok (camera_kernels.hip), on the values as the fp32 struct holds them."""
        f32 = lambda x: C.c_float(float(x)).value      # noqa: E731
        if int(self.width) <= 0 or int(self.height) <= 0:
            raise ValueError("camera width and height must be positive")
        if not (math.isfinite(f32(self.focal_length)) and math.isfinite(f32(self.horizontal_aperture)) and
                f32(self.focal_length) > 0 and f32(self.horizontal_aperture) > 0):
            raise ValueError("camera focal_length and horizontal_aperture must be positive and finite")
        if self.vertical_aperture is not None and not (math.isfinite(f32(self.vertical_aperture)) and f32(self.vertical_aperture) > 0):
            raise ValueError("camera vertical_aperture must be positive and finite, or None (square pixels)")
        if not (0 <= f32(self.near_clip) < f32(self.far_clip)):
            raise ValueError("camera clipping range must satisfy 0 <= near_clip < far_clip (far_clip may be inf)")
        if len(self.position) != 3 or len(self.orientation) != 4 or not any(f32(q) != 0.0 for q in self.orientation):
            raise ValueError("camera position must be (x, y, z) and orientation a non-zero (w, x, y, z) quaternion")
        if not all(math.isfinite(f32(v)) for v in (*self.position, *self.orientation)):
            raise ValueError("camera position and orientation must be finite")
        if int(self.every_n_steps) < 1:
            raise ValueError("camera every_n_steps must be >= 1")
        if self.noise is not None or self.clip is not None:
            from .obs_post import image_segments
            if int(self.width) * int(self.height) > _lib.OBS_POST_MAX_WIDTH:
                raise ValueError(f"camera noise / clip need height * width <= {_lib.OBS_POST_MAX_WIDTH}")
            image_segments(self)                       # ValueError for a noise object or clip the kernel cannot run
        if self.sensor is not None:
            if int(self.width) * int(self.height) > _lib.DEPTH_SENSOR_MAX_PIXELS:
                raise ValueError(f"a camera sensor needs height * width <= {_lib.DEPTH_SENSOR_MAX_PIXELS}")
            self.sensor.to_native(self.focal_px[0])    # ValueError for a parameter the kernel refuses

    def to_native(self) -> "_lib.CameraConfig":
        self.validate()
        c = _lib.CameraConfig()
        c.width, c.height = int(self.width), int(self.height)
        c.focal_length, c.horizontal_aperture = self.focal_length, self.horizontal_aperture
        c.vertical_aperture = 0.0 if self.vertical_aperture is None else self.vertical_aperture
        for i in range(3):
            c.mount_pos[i] = self.position[i]
        for i in range(4):
            c.mount_quat[i] = self.orientation[i]
        c.near_clip, c.far_clip = self.near_clip, self.far_clip
        return c


@dataclass
class LidarCfg:
    """A scanning lidar on the Body link in the vocabulary of ORBIT's ``patterns.LidarPatternCfg`` (include/rover_lidar.h,
    lidar.py): ``channels`` rings between the two ``vertical_fov_range`` angles (inclusive), each with one ray every
    ``horizontal_res`` degrees from ``horizontal_fov_range[0]`` on; the end of the span is left out when the span is a full circle
    and kept otherwise.  The default pattern is a free choice (a downward fan that covers the policy's 3 m x 3 m scan from the
    mast), not a particular instrument."""
    channels: int = 32
    vertical_fov_range: tuple = (-60.0, -10.0)         # degrees, elevation above the sensor's x-y plane
    horizontal_fov_range: tuple = (-180.0, 180.0)      # degrees, azimuth about the sensor's +z, 0 = +x
    horizontal_res: float = 2.0                        # degrees
    position: tuple = CameraCfg.position               # m, Body frame: the camera's mast
    orientation: tuple = (1.0, 0.0, 0.0, 0.0)          # (w, x, y, z) Body <- sensor; folded into the ray table
    near_clip: float = 0.0                             # m
    max_distance: float = 100.0                        # m, ORBIT's RayCasterCfg.max_distance; may be inf
    attach_yaw_only: bool = False                      # the table turns with the yaw frame only (ORBIT's RayCasterCfg switch)
    every_n_steps: int = 1                             # cast on steps with common_step_counter % every_n_steps == 0
    hits: bool = False                                 # extras["lidar_hits_w"]: ORBIT's ray_hits_w
    # noise on the ranges, then a clip (obs_post.py under the lidar's own stream tag, draws keyed as the camera's); both None =
    # the ranges as cast, nothing launched.  Misses stay +inf unless a clip brings them to its upper bound.
    noise: Any = None
    clip: Any = None

    @property
    def azimuth_angles(self) -> list:
        """The azimuths of one ring in degrees (float64): h0 + res * k."""
        h0, h1, res = float(self.horizontal_fov_range[0]), float(self.horizontal_fov_range[1]), float(self.horizontal_res)
        if not (math.isfinite(h0) and math.isfinite(h1) and math.isfinite(res) and res > 0.0 and h1 >= h0):
            raise ValueError("lidar horizontal_fov_range must be finite with min <= max and horizontal_res finite and > 0")
        n = int(math.floor((h1 - h0) / res + 1e-9)) + 1
        full = abs((h1 - h0) - 360.0) < 1e-9
        return [h0 + res * k for k in range(n) if not (full and h0 + res * k >= h1 - 1e-9)]

    @property
    def azimuths(self) -> int:
        return len(self.azimuth_angles)

    @property
    def rays(self) -> int:
        return int(self.channels) * self.azimuths

    def validate(self):
        """The checks of rover_lidar_cast (lidar_kernels.hip), on the values as the fp32 struct holds them."""
        f32 = lambda x: C.c_float(float(x)).value      # noqa: E731
        if int(self.channels) != self.channels or int(self.channels) < 1:
            raise ValueError("lidar channels must be an integer >= 1")
        if len(tuple(self.vertical_fov_range)) != 2 or not all(math.isfinite(float(v)) for v in self.vertical_fov_range):
            raise ValueError("lidar vertical_fov_range must be two finite angles")
        if self.rays < 1 or self.rays > 0x7FFFFFFF:
            raise ValueError("the lidar pattern must hold at least one ray")
        if len(tuple(self.position)) != 3 or not all(math.isfinite(f32(v)) for v in self.position):
            raise ValueError("lidar position must be three finite values")
        if len(tuple(self.orientation)) != 4 or not all(math.isfinite(float(q)) for q in self.orientation) or \
                not any(float(q) != 0.0 for q in self.orientation):
            raise ValueError("lidar orientation must be a finite, non-zero (w, x, y, z) quaternion")
        if not (0 <= f32(self.near_clip) < f32(self.max_distance)):
            raise ValueError("lidar range must satisfy 0 <= near_clip < max_distance (max_distance may be inf)")
        if int(self.every_n_steps) < 1:
            raise ValueError("lidar every_n_steps must be >= 1")
        if self.noise is not None or self.clip is not None:
            from .obs_post import lidar_segments
            if self.rays > _lib.OBS_POST_MAX_WIDTH:
                raise ValueError(f"lidar noise / clip need at most {_lib.OBS_POST_MAX_WIDTH} rays")
            lidar_segments(self)                       # ValueError for a noise object or clip the kernel cannot run

    def to_native(self) -> "_lib.LidarConfig":
        self.validate()
        c = _lib.LidarConfig()
        c.rays = self.rays
        for i in range(3):
            c.mount_pos[i] = self.position[i]
        c.near_clip, c.far_clip = self.near_clip, self.max_distance
        c.attach_yaw_only = 1 if self.attach_yaw_only else 0
        return c


@dataclass
class ViewerCfg:
    """The rgb_array viewer (``RoverEnv(render_mode="rgb_array").render()``): ORBIT's ``ViewerCfg`` (eye, lookat, resolution,
    origin) with the lens of Kit's default perspective camera; the image contract is DESIGN.md section 11 (include/rover_viewer.h)."""
    eye: tuple = (7.5, 7.5, 7.5)                       # m (ORBIT ViewerCfg)
    lookat: tuple = (0.0, 0.0, 0.0)
    resolution: tuple = (1280, 720)                    # (width, height) pixels
    origin_type: str = "world"                         # "world" | "env": eye and lookat relative to env `env_index`'s root position
    env_index: int = 0
    # Kit's default /OmniverseKit_Persp camera, which ORBIT's viewport renders from (an assumption: the values of that prim as Kit
    # creates it, not in the reference checkout): horizontal FOV 2 atan(20.955 / (2 x 18.147562)) = 60.0 deg, square pixels
    focal_length: float = 18.147562                    # mm
    horizontal_aperture: float = 20.955                # mm
    near_clip: float = 0.01                            # m
    far_clip: float = 1000000.0                        # m; may be inf
    draw_targets: bool = True                          # one sphere per env at its target (the command term's debug_vis=True)

    def validate(self, num_envs: int | None = None):
        """The checks of the library's config_ok (viewer_kernels.hip), on the values as the fp32 struct holds them; the env index
        is checked against ``num_envs`` when it is given."""
        f32 = lambda x: C.c_float(float(x)).value      # noqa: E731
        if len(self.eye) != 3 or len(self.lookat) != 3:
            raise ValueError("viewer eye and lookat must be (x, y, z)")
        eye, at = [f32(v) for v in self.eye], [f32(v) for v in self.lookat]
        if not all(math.isfinite(v) for v in eye + at):
            raise ValueError("viewer eye and lookat must be finite")
        if at[0] - eye[0] == 0.0 and at[1] - eye[1] == 0.0:
            raise ValueError("viewer lookat - eye must have a horizontal component (eye == lookat, or a view along the Z axis)")
        if len(self.resolution) != 2 or not all(1 <= int(x) <= _lib.VIEWER_MAX_SIZE for x in self.resolution):
            raise ValueError(f"viewer resolution must be (width, height), each in 1 .. {_lib.VIEWER_MAX_SIZE}")
        if not (math.isfinite(f32(self.focal_length)) and math.isfinite(f32(self.horizontal_aperture)) and
                f32(self.focal_length) > 0 and f32(self.horizontal_aperture) > 0):
            raise ValueError("viewer focal_length and horizontal_aperture must be positive and finite")
        if not (0 <= f32(self.near_clip) < f32(self.far_clip)):
            raise ValueError("viewer clipping range must satisfy 0 <= near_clip < far_clip (far_clip may be inf)")
        if self.origin_type not in ("world", "env"):
            raise ValueError("viewer origin_type must be 'world' or 'env'")
        if self.origin_type == "env" and (int(self.env_index) < 0 or (num_envs is not None and int(self.env_index) >= num_envs)):
            raise ValueError(f"viewer env_index {self.env_index} is out of range for {num_envs} envs")

    def to_native(self, num_envs: int | None = None) -> "_lib.ViewerConfig":
        self.validate(num_envs)
        c = _lib.ViewerConfig()
        for i in range(3):
            c.eye[i], c.lookat[i] = self.eye[i], self.lookat[i]
        c.origin_type = _lib.VIEWER_ORIGIN_ENV if self.origin_type == "env" else _lib.VIEWER_ORIGIN_WORLD
        c.env_index = int(self.env_index)
        c.width, c.height = int(self.resolution[0]), int(self.resolution[1])
        c.focal_length, c.horizontal_aperture = self.focal_length, self.horizontal_aperture
        c.near_clip, c.far_clip = self.near_clip, self.far_clip
        c.draw_targets = int(bool(self.draw_targets))
        return c


def _default_observations():
    return {
        "actions": TermCfg("last_action"),
        "distance": TermCfg("distance_to_target_euclidean", scale=0.11, params={"command_name": "target_pose"}),
        "heading": TermCfg("angle_to_target_observation", scale=1 / math.pi, params={"command_name": "target_pose"}),
        "height_scan": TermCfg("height_scan_rover", scale=1, params={"sensor_cfg": "height_scanner"}),
    }


def _default_rewards():
    return {
        "distance_to_target": TermCfg("distance_to_target_reward", weight=5.0, params={"command_name": "target_pose"}),
        "reached_target": TermCfg("reached_target", weight=5.0, params={"command_name": "target_pose", "threshold": 0.18}),
        "oscillation": TermCfg("oscillation_penalty", weight=-0.1),
        "angle_to_target": TermCfg("angle_to_target_penalty", weight=-1.5, params={"command_name": "target_pose"}),
        "heading_soft_contraint": TermCfg("heading_soft_contraint", weight=-0.5, params={"asset_cfg": "robot"}),
        "collision": TermCfg("collision_penalty", weight=-2.0, params={"sensor_cfg": "contact_sensor", "threshold": 1.0}),
        "far_from_target": TermCfg("far_from_target_reward", weight=-2.0, params={"command_name": "target_pose", "threshold": 11.0}),
    }


def _default_terminations():
    return {
        "time_limit": TermCfg("time_out", time_out=True),
        "is_success": TermCfg("is_success", params={"command_name": "target_pose", "threshold": 0.18}),
        "far_from_target": TermCfg("far_from_target", params={"command_name": "target_pose", "threshold": 11.0}),
        "collision": TermCfg("collision_with_obstacles", params={"sensor_cfg": "contact_sensor", "threshold": 1.0}),
    }


REWARD_ORDER = ["distance_to_target", "reached_target", "oscillation", "angle_to_target", "heading_soft_contraint",
                "collision", "far_from_target"]
REWARD_FUNCS = ["distance_to_target_reward", "reached_target", "oscillation_penalty", "angle_to_target_penalty",
                "heading_soft_contraint", "collision_penalty", "far_from_target_reward"]
TERMINATION_ORDER = ["time_limit", "is_success", "far_from_target", "collision"]
TERMINATION_FUNCS = ["time_out", "is_success", "far_from_target", "collision_with_obstacles"]
OBS_ORDER = ["actions", "distance", "heading", "height_scan"]
OBS_FUNCS = ["last_action", "distance_to_target_euclidean", "angle_to_target_observation", "height_scan_rover"]


@dataclass
class RoverEnvCfg:
    scene: SceneCfg = field(default_factory=SceneCfg)
    sim: SimCfg = field(default_factory=SimCfg)
    decimation: int = 6                      # rover_env_cfg.py:270
    episode_length_s: float = 150.0          # rover_env_cfg.py:271
    height_scanner: RayCasterCfg = field(default_factory=RayCasterCfg)
    actions: AckermannActionCfg = field(default_factory=AckermannActionCfg)
    commands: CommandCfg = field(default_factory=CommandCfg)
    observations: dict = field(default_factory=_default_observations)
    rewards: dict = field(default_factory=_default_rewards)
    terminations: dict = field(default_factory=_default_terminations)
    terrain: TerrainCfg = field(default_factory=TerrainCfg)
    reset_z_offset: float = 0.5              # randomizations.py:12
    reset_velocities: str = "reference"      # "reference" (root pose only, B-17) | "zero"
    # spawn row of a reset (randomizations.py:22 draws a randperm prefix): "distinct" = no two envs reset in the same call
    # share a row (like the reference), "independent" = one uniform draw per env (rows may repeat)
    spawn_draw: str = "distinct"
    seed: int = 0
    friction: float = 0.75
    solver_iterations: int = 32             # Jacobi sweeps of the contact solver = the reference's solver_position_iteration_count
                                            # (aau_rover_simple.py:33); rounds 1-4 ran 16
    # where the rover's 25 kg act: "subtree_weights" = the weight of each bogie subtree (beam + steer links + wheels: 7 + 7 + 9 kg
    # of the USD link table) at its own centre of mass -- the static wheel loads of the articulated rover; "lumped" = rounds 1-4
    mass_model: str = "subtree_weights"
    step_mapping: str = "auto"              # "auto" | "lane" (one env per lane) | "group" (sixteen lanes per env)
    record_contact_forces: bool = True       # materialise contact_sensor.data.force_matrix_w every step
    use_int16_terrain: bool = True           # stage the exact int16 copy of the heightfield in the scan kernel when it exists
    roctx_markers: bool = False              # roctx ranges around the two launches of every step (rocprofv3 --marker-trace)
    # extras["log"]: "on_demand" = the reduction of the episodic sums runs when the dictionary is read (same numbers; lets a step be
    # ONE kernel launch where the fused step + scan kernel applies); "every_step" = behind every step, like the C entry's default
    log_reduction: str = "on_demand"
    # observation rows written with streaming (non-temporal) stores by the one-launch kernels: ~2 % faster step when nothing on the
    # device reads the rows next; off by default because a policy kernel behind the step finds plainly stored rows in L2
    stream_observations: bool = False
    log_values: str = "device"              # extras["log"] entries: 0-d device tensors (ORBIT) | "host": views of a pinned mirror, ONE
                                            # synchronisation per step for a trainer that .item()s every entry (skrl_utils.py:139-142)
    # who finishes the terms of observation_post(): "torch" = a few torch ops per term and step, draws from the env's own
    # torch.Generator; "fused" = one HIP launch (obs_post.py), draws keyed by (seed, global env id, call counter, column), so
    # they survive a split over ranks and a checkpoint
    observation_post_backend: str = "torch"
    # multi-GPU sharding: this process simulates global env ids [env_id_offset, env_id_offset + num_envs)
    env_id_offset: int = 0
    global_num_envs: int | None = None
    # the on-board depth camera (RoverEnvCamera): None = no camera, nothing rendered
    camera: CameraCfg | None = None
    # a rolling elevation map fed by the camera (elevation.py): None = no map, nothing launched.  With one, extras["elevation_scan"]
    # is the height scan read out of the map, beside extras["elevation_known"] and extras["elevation_count"]
    elevation: ElevationMapCfg | None = None
    # a scanning lidar (lidar.py): None = no lidar, no key, buffer or launch.  With one, extras["lidar_range"] is the
    # (num_envs, channels, azimuths) range frame, +inf on a miss; cfg.elevation.source = "lidar" builds the map from it
    lidar: LidarCfg | None = None
    # the rgb_array viewer's camera (render_mode="rgb_array"): ORBIT's ViewerCfg defaults
    viewer: ViewerCfg = field(default_factory=ViewerCfg)

    # ------------------------------------------------------------------------------------------------------------
    def custom_terms(self, table: dict, order: list) -> dict:
        """The user-written entries of a term table: everything beside the built-in names, ``func`` a callable."""
        return {k: t for k, t in table.items() if k not in order}

    @property
    def has_custom_terms(self) -> bool:
        return bool(self.custom_terms(self.rewards, REWARD_ORDER) or self.custom_terms(self.terminations, TERMINATION_ORDER))

    def validate(self):
        for table, order, funcs, what in ((self.rewards, REWARD_ORDER, REWARD_FUNCS, "reward"),
                                          (self.terminations, TERMINATION_ORDER, TERMINATION_FUNCS, "termination"),
                                          (self.observations, OBS_ORDER, OBS_FUNCS, "observation")):
            builtin = [k for k in table if k in order]
            if builtin != order:
                raise ValueError(f"the built-in {what} terms {order} must all be present, in this order (fused in the HIP kernels; "
                                 f"switch a reward off with weight=0); got {list(table)}")
            for name, fn in zip(order, funcs):
                if table[name].func != fn:
                    raise ValueError(f"{what} term '{name}' must use func '{fn}' (got '{table[name].func}')")
            for name, t in self.custom_terms(table, order).items():
                if what == "observation":
                    raise ValueError(f"observation term '{name}': the observation row is fixed (4 + rays columns, the layout the policy "
                                     "checkpoint expects); user-written terms are supported for rewards and terminations")
                if not callable(t.func):
                    raise ValueError(f"{what} term '{name}': func must be a callable func(env, **params) (got {t.func!r}); the built-in "
                                     f"{what} terms are {order}")
        if self.reset_velocities not in ("reference", "zero"):
            raise ValueError("reset_velocities must be 'reference' or 'zero'")
        if self.spawn_draw not in ("distinct", "independent"):
            raise ValueError("spawn_draw must be 'distinct' or 'independent'")
        if self.log_values not in ("device", "host"):
            raise ValueError("log_values must be 'device' or 'host'")
        if self.mass_model not in ("lumped", "subtree_weights"):
            raise ValueError("mass_model must be 'subtree_weights' or 'lumped'")
        if self.observation_post_backend not in ("torch", "fused"):
            raise ValueError("observation_post_backend must be 'torch' or 'fused'")
        if self.observation_post_backend == "fused" and self.observation_post():
            from .obs_post import segments
            segments(self)                             # ValueError for a noise object the kernel cannot run
        if self.commands.simple_heading:
            raise ValueError("simple_heading=True is not supported (the reference cfg uses False, rover_env_cfg.py:195)")
        if self.camera is not None:
            self.camera.validate()
        if self.lidar is not None:
            self.lidar.validate()
        if self.elevation is not None and self.elevation.source not in ("camera", "lidar"):
            raise ValueError("elevation source must be 'camera' or 'lidar'")
        if self.elevation is not None and self.elevation.source == "lidar":
            if self.lidar is None:
                raise ValueError("cfg.elevation.source = 'lidar' needs cfg.lidar: the map is built from the range frame")
            if self.lidar.attach_yaw_only:
                raise ValueError("an elevation map from the lidar needs attach_yaw_only = False: the map unprojects with the full attitude")
            if self.lidar.rays > _lib.ELEVATION_MAX_PIXELS:
                raise ValueError(f"an elevation map needs at most {_lib.ELEVATION_MAX_PIXELS} lidar rays")
            nx, ny = self.height_scanner.grid
            if nx * ny > _lib.ELEVATION_MAX_RAYS:
                raise ValueError(f"an elevation map needs at most {_lib.ELEVATION_MAX_RAYS} scan rays")
            self.elevation.to_native(self.lidar.position, self.height_scanner.height_offset)
        elif self.elevation is not None:
            if self.camera is None:
                raise ValueError("cfg.elevation needs cfg.camera: the map is built from the depth image")
            if int(self.camera.width) * int(self.camera.height) > _lib.ELEVATION_MAX_PIXELS:
                raise ValueError(f"an elevation map needs camera height * width <= {_lib.ELEVATION_MAX_PIXELS}")
            nx, ny = self.height_scanner.grid
            if nx * ny > _lib.ELEVATION_MAX_RAYS:
                raise ValueError(f"an elevation map needs at most {_lib.ELEVATION_MAX_RAYS} scan rays")
            self.elevation.to_native(self.camera.position, self.height_scanner.height_offset)
        self.viewer.validate(self.scene.num_envs)

    def observation_post(self) -> dict:
        """Observation terms whose ORBIT post-processing (ObservationManager.compute_group: noise, then clip, then scale) is not
        what the kernels compute: any ``noise`` / ``clip``, or a ``scale`` != 1 on ``actions`` / ``height_scan`` (the kernels scale
        ``distance`` and ``heading`` only).  For these the kernels write the raw term (scale 1) and ``RoverEnv`` finishes the columns
        in torch (three small ops per term and step: not the one-launch fast path any more, but the same step kernel).
        With ``observation_post_backend = "fused"`` one HIP launch behind the step kernel finishes them instead (obs_post.py)."""
        out = {}
        for name in OBS_ORDER:
            t = self.observations[name]
            if t.noise is not None or t.clip is not None or (name in ("actions", "height_scan") and float(t.scale) != 1.0):
                if t.clip is not None and len(tuple(t.clip)) != 2:
                    raise ValueError(f"observation term '{name}': clip must be (min, max)")
                out[name] = t
        return out

    @property
    def max_episode_length(self) -> int:
        # ORBIT: ceil(episode_length_s / (sim.dt * decimation))
        return math.ceil(self.episode_length_s / (self.sim.dt * self.decimation))

    def to_native(self) -> "_lib.RoverConfig":
        self.validate()
        c = _lib.default_config()
        a = self.actions
        off = a.offset if isinstance(a.offset, (tuple, list)) else (a.offset, a.offset)
        c.scale_lin, c.scale_ang = float(a.scale[0]), float(a.scale[1])
        c.offset_lin, c.offset_ang = float(off[0]), float(off[1])
        c.wheel_radius, c.d_fr = a.wheel_radius, a.rear_and_front_wheel_distance
        c.d_mw, c.wheelbase = a.middle_wheel_distance, a.wheelbase_length
        c.sim_dt, c.decimation = self.sim.dt, self.decimation
        c.max_episode_length = self.max_episode_length
        c.max_episode_length_s = self.episode_length_s
        # four independent table entries in the reference (rover_env_cfg.py:136, 162 rewards; :173, 177 terminations)
        c.success_threshold = self.terminations["is_success"].params["threshold"]
        c.far_threshold = self.terminations["far_from_target"].params["threshold"]
        c.rew_success_threshold = self.rewards["reached_target"].params["threshold"]
        c.rew_far_threshold = self.rewards["far_from_target"].params["threshold"]
        c.target_distance = self.commands.target_distance
        c.heading_lo, c.heading_hi = self.commands.heading_range
        if self.commands.resampling_time_range[0] != self.commands.resampling_time_range[1]:
            raise ValueError("resampling_time_range must be a single value (rover_env_cfg.py:196)")
        c.resample_time = self.commands.resampling_time_range[0]
        for i, name in enumerate(REWARD_ORDER):
            c.rew_weight[i] = self.rewards[name].weight
        post = self.observation_post()         # terms finished in torch get their raw value from the kernels
        c.obs_scale_distance = 1.0 if "distance" in post else self.observations["distance"].scale
        c.obs_scale_heading = 1.0 if "heading" in post else self.observations["heading"].scale
        hs = self.height_scanner
        c.scan_resolution, c.scan_size_x, c.scan_size_y = hs.resolution, hs.size[0], hs.size[1]
        c.scan_nx, c.scan_ny = hs.grid
        c.scan_height_offset = hs.height_offset
        c.scan_surface = {"triangles": 0, "bilinear": 1}[hs.surface]
        c.reset_z_offset = self.reset_z_offset
        c.reset_mode = 0 if self.reset_velocities == "reference" else 1
        c.spawn_draw = {"independent": 0, "distinct": 1}[self.spawn_draw]
        c.seed_lo, c.seed_hi = self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF
        c.friction_mu = self.friction
        c.solver_iterations = self.solver_iterations
        c.mass_model = {"lumped": 0, "subtree_weights": 1}[self.mass_model]
        c.max_target_tries = self.commands.max_target_tries
        c.step_mapping = {"auto": 0, "lane": 1, "group": 2}[self.step_mapping]
        return c


@dataclass
class AAURoverEnvCfg(RoverEnvCfg):
    """``AAURoverEnv-v0`` (robots/aau_rover/env_cfg.py:10-31): the defaults above already are the AAU values, and the viewer's eye
    is the one rover_env_cfg.py:272 sets."""
    viewer: ViewerCfg = field(default_factory=lambda: ViewerCfg(eye=(-6.0, -6.0, 3.5)))


@dataclass
class AAURoverCameraEnvCfg(AAURoverEnvCfg):
    """``RoverCamera-v0`` (rover_envs/envs/__init__.py:38-42, rover_camera_env.py:18-76): the AAU rover with its depth camera."""
    camera: CameraCfg | None = field(default_factory=CameraCfg)
