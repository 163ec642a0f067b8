"""What the lidar's GPU tests share: a rig that casts any table from any poses over any terrain through the C ABI, the float64
reference of those rays and the project's comparison rule (tests/test_gpu_camera_edges.py::_check), restated for ranges."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from camera_reference import cast, cast_brute
from isaac_rover_orbit_amd import _lib, lidar
from isaac_rover_orbit_amd import terrain as T
from isaac_rover_orbit_amd.cfg import LidarCfg, RoverEnvCfg

DEV = "cuda:0"
ERR_INVALID, ERR_STATE = 1, 2


def quat(yaw, pitch=0.0, roll=0.0):
    cy, sy, cp, sp, cr, sr = (math.cos(yaw / 2), math.sin(yaw / 2), math.cos(pitch / 2), math.sin(pitch / 2),
                              math.cos(roll / 2), math.sin(roll / 2))
    return [cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy]


def dense_cfg(**kw):
    """64 channels over -85 ... -20 degrees, 1.5 degrees of azimuth: 15360 rays."""
    return LidarCfg(channels=64, vertical_fov_range=(-85.0, -20.0), horizontal_res=1.5, **kw)


def flat_terrain(shape=(256, 256), min_x=0.0, min_y=0.0):
    """Flat ground with every spawn in the middle."""
    zero = np.zeros(shape, np.float32)
    ter = T.Terrain(ground=zero, obstacle=zero.copy(), min_x=min_x, min_y=min_y, rock_mask=zero.astype(np.uint8),
                    safe_rock_mask=zero.astype(np.uint8))
    sp = np.zeros((4096, 3), np.float32)
    sp[:, 0], sp[:, 1] = min_x + 0.5 * (shape[1] - 1) * T.RESOLUTION, min_y + 0.5 * (shape[0] - 1) * T.RESOLUTION
    ter.spawn_locations = sp
    return ter


def make_env(terrain, n, **cfg_fields):
    from isaac_rover_orbit_amd.envs import RoverEnv
    cfg = RoverEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.terrain.kind = "custom"
    for k, v in cfg_fields.items():
        setattr(cfg, k, v)
    return RoverEnv(cfg, terrain=terrain)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def rough(shape, seed, amp=0.25):
    """Random heights with some relief: smooth waves plus per-node noise (a rough surface on which the diagonal matters)."""
    rng = np.random.default_rng(seed)
    H, W = shape
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    h = amp * (np.sin(i / 7.0 + 0.3) * np.cos(j / 9.0) + 0.5 * np.sin((i + 2 * j) / 13.0)) + rng.normal(0.0, 0.4 * amp, shape)
    return h.astype(np.float32)


def random_table(R, seed, down=True):
    """R unit directions, mostly downward, float32 of the float64 unit vector."""
    g = np.random.default_rng(seed)
    d = g.normal(size=(R, 3))
    if down:
        d[:, 2] = -np.abs(d[:, 2]) - 0.2
    return np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True), dtype=np.float32)


class Rig:
    """A sensor-less env whose handle gets any terrain (rover_set_terrain) and any states, and casts any table through the C ABI.
    Nothing steps after a terrain is bound here, so the env's scanner never reads it."""

    def __init__(self, n):
        self.n = n
        self.env = make_env(flat_terrain(), n)
        self.lib, self.h = self.env._lib, self.env._h
        self.ws = None

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def bind(self, height, res, min_x, min_y):
        height = np.ascontiguousarray(height, np.float32)
        H, W = height.shape
        self.height, self.res, self.min_x, self.min_y = height, float(res), float(min_x), float(min_y)
        self._dev = [torch.from_numpy(height).to(DEV), torch.zeros(H, W, device=DEV), torch.zeros(H, W, dtype=torch.uint8, device=DEV)]
        sp = self.env._spawns_dev
        rc = self.lib.rover_set_terrain(self.h, ptr(self._dev[0]), ptr(self._dev[1]), ptr(self._dev[2]), H, W, self.res, self.min_x,
                                        self.min_y, ptr(sp), int(sp.shape[0]))
        assert rc == 0, self.lib.rover_last_error()
        self.ws = None

    def prepare(self):
        nb = int(self.lib.rover_lidar_workspace_bytes(self.h))
        assert nb > 0
        self.ws = torch.zeros((nb + 3) // 4, dtype=torch.float32, device=DEV)
        assert self.lib.rover_lidar_prepare(self.h, ptr(self.ws), nb, self.stream()) == 0, self.lib.rover_last_error()

    def set_poses(self, pos, quat_):
        """Body poses (n, 3), (n, 4) into the state; returns them as the float32 state holds them."""
        S = self.env.get_state().clone()
        S[:, _lib.POS:_lib.POS + 3] = torch.as_tensor(np.asarray(pos, np.float32))
        S[:, _lib.QUAT:_lib.QUAT + 4] = torch.as_tensor(np.asarray(quat_, np.float32))
        self.env.set_state(S)
        return np.asarray(pos, np.float32), np.asarray(quat_, np.float32)

    def cast(self, cfg, table, hits=False, gap=0):
        """(range (n, R) numpy, hits (n, R, 3) numpy or None, the whole NaN-filled range allocation (n, R + gap)) of the states
        set last; ``table`` (R, 3) float32, ``cfg`` a LidarCfg whose pattern is ignored."""
        if self.ws is None:
            self.prepare()
        R = int(table.shape[0])
        c = cfg.to_native()
        c.rays = R
        tab = torch.from_numpy(np.ascontiguousarray(table, np.float32)).to(DEV)
        buf = torch.full((self.n, R + gap), float("nan"), dtype=torch.float32, device=DEV)
        hb = torch.full((self.n, R, 3), float("nan"), dtype=torch.float32, device=DEV) if hits else None
        rc = self.lib.rover_lidar_cast(self.h, C.byref(c), ptr(self.ws), ptr(tab), ptr(buf), R + gap, ptr(hb), self.stream())
        assert rc == 0, self.lib.rover_last_error()
        whole = buf.cpu().numpy()
        return whole[:, :R], (None if hb is None else hb.cpu().numpy()), whole

    def close(self):
        self.env.close()


def reference(cfg, table, height, res, min_x, min_y, pos, quat_):
    """(range, clearance, origins, directions): cast_brute and cast's clearance in float64 on the specification's float32
    world_rays of poses ``pos`` / ``quat_``, each (n, R)."""
    o, d = lidar.world_rays(cfg, table, pos, quat_)
    n, R = d.shape[0], d.shape[1]
    org = np.repeat(o[:, None, :], R, 1).reshape(-1, 3).astype(np.float64)
    dd = d.reshape(-1, 3).astype(np.float64)
    near, far = float(np.float32(cfg.near_clip)), float(np.float32(cfg.max_distance))
    ok = np.isfinite(org).all(1) & np.isfinite(dd).all(1)       # a non-finite ray is a miss by the header
    ref, clear = np.full(n * R, np.inf), np.full(n * R, np.inf)
    if ok.any():
        _, clear[ok] = cast(height, res, min_x, min_y, org[ok], dd[ok], near, far)
        ref[ok] = cast_brute(height, res, min_x, min_y, org[ok], dd[ok], near, far)
    return ref.reshape(n, R), clear.reshape(n, R), o, d


def check(gpu, ref, clear, share=0.0005, what=""):
    """The project's rule: hit and miss agree and |r - ref| <= 1e-4 ref + 1e-4; a ray that fails is a grazing one (clearance
    <= 1 mm), and there are at most ``share * size + 2`` of them (share = 0: the targeted tests, where only grazing rays may
    differ at all, however many)."""
    g = gpu.astype(np.float64)
    same = np.isfinite(g) == np.isfinite(ref)
    fin = same & np.isfinite(ref)
    ok = same.copy()
    ok[fin] = np.abs(g[fin] - ref[fin]) <= 1e-4 * ref[fin] + 1e-4
    bad = ~ok
    nb = int(bad.sum())
    assert (clear[bad] <= 1e-3).all(), (f"{what}: {nb} rays disagree, {int((clear[bad] > 1e-3).sum())} of them not grazing; "
                                        f"first at {np.argwhere(bad & (clear > 1e-3))[0].tolist()}")
    if share:
        assert nb <= share * g.size + 2, f"{what}: {nb} of {g.size} rays disagree"
    return nb
