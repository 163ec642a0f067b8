"""Depth camera on the MI355X at its edges: terrain shapes whose pyramid blocks are cut short, spikes on block boundaries, every
camera setting, exactly axis-aligned rays, poses outside / above / below the terrain, degenerate states, the bench workload,
output past 2^31 elements and the refusals of the C ABI.

The yardstick is ``camera_reference.cast_brute`` (every ray against the mesh's triangle list) on small terrains and the DDA
reference ``cast`` on large ones (itself pinned to ``cast_brute`` by tests/test_camera.py), under the rule of
test_gpu_camera._compare_to_reference: hit / miss agree and |depth - ref| <= 1e-4 d + 1e-4, and a pixel that does not is a
grazing one (clearance <= 1 mm).  Terrains other than the env's own are bound through rover_set_terrain on the env's handle."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from camera_reference import camera_rays, cast, cast_brute
from isaac_rover_orbit_amd import _lib
from isaac_rover_orbit_amd import terrain as T
from isaac_rover_orbit_amd.cfg import CameraCfg, RoverEnvCfg
from oracle.mesh_raycast import heightfield_mesh, vertical_ray_hits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ERR_INVALID, ERR_STATE = 1, 2


def _quat(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = (math.cos(yaw / 2), math.sin(yaw / 2), math.cos(pitch / 2), math.sin(pitch / 2),
                              math.cos(roll / 2), math.sin(roll / 2))
    return [cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy]


def _flat_terrain(shape=(256, 256), min_x=0.0, min_y=0.0):
    """Flat ground with every spawn in the middle (the env's own terrain where the tests bind another or do not look)."""
    zero = np.zeros(shape, np.float32)
    ter = T.Terrain(ground=zero, obstacle=zero.copy(), min_x=min_x, min_y=min_y, rock_mask=zero.astype(np.uint8),
                    safe_rock_mask=zero.astype(np.uint8))
    sp = np.zeros((4096, 3), np.float32)
    sp[:, 0], sp[:, 1] = min_x + 0.5 * (shape[1] - 1) * T.RESOLUTION, min_y + 0.5 * (shape[0] - 1) * T.RESOLUTION
    ter.spawn_locations = sp
    return ter


def _env(terrain, n, camera=None, device=DEV):
    from isaac_rover_orbit_amd.envs import RoverEnv
    cfg = RoverEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = device
    cfg.terrain.kind = "custom"
    cfg.camera = camera
    return RoverEnv(cfg, terrain=terrain)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class Rig:
    """A camera-less env whose handle gets any terrain (rover_set_terrain), any camera config and any states, and renders through
    the C ABI.  Nothing steps after a terrain is bound here, so the env's scanner never reads it."""

    def __init__(self, n):
        self.n = n
        self.env = _env(_flat_terrain(), n)
        self.lib, self.h = self.env._lib, self.env._h
        self.ws = None

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def bind(self, height, res, min_x, min_y):
        height = np.ascontiguousarray(height, np.float32)
        H, W = height.shape
        self.height = height
        self.res, self.min_x, self.min_y = float(res), float(min_x), float(min_y)
        self._dev = [torch.from_numpy(height).to(DEV), torch.zeros(H, W, device=DEV), torch.zeros(H, W, dtype=torch.uint8, device=DEV)]
        sp = self.env._spawns_dev
        rc = self.lib.rover_set_terrain(self.h, _ptr(self._dev[0]), _ptr(self._dev[1]), _ptr(self._dev[2]), H, W, self.res,
                                        self.min_x, self.min_y, _ptr(sp), int(sp.shape[0]))
        assert rc == 0, self.lib.rover_last_error()
        self.ws = None

    def prepare(self, cam):
        cfg = cam.to_native()
        nb = int(self.lib.rover_camera_workspace_bytes(self.h, C.byref(cfg)))
        assert nb > 0
        self.ws = torch.zeros((nb + 3) // 4, dtype=torch.float32, device=DEV)
        assert self.lib.rover_camera_prepare(self.h, C.byref(cfg), _ptr(self.ws), nb, self.stream()) == 0, self.lib.rover_last_error()

    def render(self, cam) -> np.ndarray:
        """(n, height, width) depth of the states set last."""
        if self.ws is None:
            self.prepare(cam)
        buf = torch.full((self.n, cam.height, cam.width), float("nan"), dtype=torch.float32, device=DEV)
        cfg = cam.to_native()
        assert self.lib.rover_camera_render(self.h, C.byref(cfg), _ptr(self.ws), _ptr(buf), self.stream()) == 0, self.lib.rover_last_error()
        return buf.cpu().numpy()

    def set_poses(self, pos, quat):
        """Body poses (n, 3), (n, 4) into the state; returns them as the fp32 state holds them, in float64."""
        S = self.env.get_state().clone()
        S[:, _lib.POS:_lib.POS + 3] = torch.as_tensor(np.asarray(pos, np.float32))
        S[:, _lib.QUAT:_lib.QUAT + 4] = torch.as_tensor(np.asarray(quat, np.float32))
        self.env.set_state(S)
        return np.asarray(pos, np.float32).astype(np.float64), np.asarray(quat, np.float32).astype(np.float64)

    def close(self):
        self.env.close()


def _reference(cam, height, res, min_x, min_y, P, Q, brute=True, pixels=None):
    """(depth, clearance), each (N, number of pixels): the reference of pixels ``pixels`` (flat indices, default all) of the
    images of body poses P, Q; the depth from cast_brute (or from cast with brute=False), the clearance from cast."""
    o, d = camera_rays(cam, P, Q)
    N = o.shape[0]
    d = d.reshape(N, -1, 3)
    if pixels is not None:
        d = d[:, pixels]
    k = d.shape[1]
    org = np.repeat(o[:, None, :], k, 1).reshape(-1, 3)
    d = d.reshape(-1, 3)
    dep, clear = cast(height, res, min_x, min_y, org, d, cam.near_clip, cam.far_clip)
    if brute:
        dep = cast_brute(height, res, min_x, min_y, org, d, cam.near_clip, cam.far_clip)
    return dep.reshape(N, k), clear.reshape(N, k)


def _check(gpu, ref, clear, share=0.0005, what=""):
    """The rule of test_gpu_camera._compare_to_reference: every failing pixel is a grazing one, and there are at most ``share``
    of them (share=0: the targeted tests, where only grazing pixels may differ at all, however many)."""
    g = gpu.astype(np.float64)
    same = np.isfinite(g) == np.isfinite(ref)
    fin = same & np.isfinite(ref)
    ok = same.copy()
    ok[fin] = np.abs(g[fin] - ref[fin]) <= 1e-4 * ref[fin] + 1e-4
    bad = ~ok
    nb = int(bad.sum())
    assert (clear[bad] <= 1e-3).all(), (f"{what}: {nb} pixels disagree, {int((clear[bad] > 1e-3).sum())} of them not grazing; "
                                        f"first at {np.argwhere(bad & (clear > 1e-3))[0].tolist()}")
    if share:
        assert nb <= share * g.size + 2, f"{what}: {nb} of {g.size} pixels disagree"


def _rough(shape, seed, amp=0.25):
    """Random heights with some relief: smooth waves plus per-node noise (a rough surface on which the diagonal matters)."""
    rng = np.random.default_rng(seed)
    H, W = shape
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    h = amp * (np.sin(i / 7.0 + 0.3) * np.cos(j / 9.0) + 0.5 * np.sin((i + 2 * j) / 13.0)) + rng.normal(0.0, 0.4 * amp, shape)
    return h.astype(np.float32)


def _surface(height, res, min_x, min_y, x, y):
    """Height of the mesh under (x, y) (float64; -inf off the terrain)."""
    V, F = heightfield_mesh(np.asarray(height, np.float64), res, min_x, min_y)
    return vertical_ray_hits(V, F, np.stack([np.asarray(x, np.float64), np.asarray(y, np.float64)], 1))


# ---------------------------------------------------------------------------------------------------------- (a) terrain shapes
@pytest.mark.parametrize("H,W,res,min_x,min_y", [(203, 331, 0.05, -7.3, 4.1), (130, 71, 0.1, 3.2, -9.0), (66, 65, 0.07, -1.0, -1.0),
                                                 (9, 2, 0.05, 0.4, -0.3), (2, 2, 0.05, -0.2, 0.35)])
def test_terrain_shapes_and_placement(H, W, res, min_x, min_y):
    """Non-square terrains with H - 1 and W - 1 not multiples of 8 or 64 (partial pyramid blocks on both levels), the smallest
    terrain rover_set_terrain accepts, negative and positive origins, resolutions other than 0.05."""
    height = _rough((H, W), seed=H * 1000 + W)
    ext_x, ext_y = (W - 1) * res, (H - 1) * res
    small = max(ext_x, ext_y) < 2.0
    if small:   # a narrow camera looking down on a terrain a few cells wide
        cam = CameraCfg(width=23, height=17, focal_length=4.0, horizontal_aperture=2.0, position=(0.0, 0.0, 0.0),
                        orientation=(1.0, 0.0, 0.0, 0.0))
    else:
        cam = CameraCfg()
    rng = np.random.default_rng(H + W)
    n = 6
    rig = Rig(n)
    rig.bind(height, res, min_x, min_y)
    top = float(height.max())
    pos, quat = [], []
    for k in range(n):
        if small:
            x, y = min_x + rng.uniform(-0.2, 1.2) * ext_x, min_y + rng.uniform(-0.2, 1.2) * ext_y
            pos.append((x, y, top + rng.uniform(0.05, 0.3)))
            quat.append(_quat(rng.uniform(-math.pi, math.pi), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)))
        else:
            x, y = min_x + rng.uniform(0.1, 0.9) * ext_x, min_y + rng.uniform(0.1, 0.9) * ext_y
            pos.append((x, y, top + rng.uniform(-0.3, 0.8)))
            quat.append(_quat(rng.uniform(-math.pi, math.pi), rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25)))
    P, Q = rig.set_poses(pos, quat)
    gpu = rig.render(cam).reshape(n, -1)
    rig.close()
    if small:
        ref, clear = _reference(cam, height, res, min_x, min_y, P, Q)
        _check(gpu, ref, clear, what="brute")
    else:
        ref, clear = _reference(cam, height, res, min_x, min_y, P, Q, brute=False)
        _check(gpu, ref, clear, what="cast")
        pix = np.random.default_rng(1).choice(gpu.shape[1], 300, replace=False)
        ref, clear = _reference(cam, height, res, min_x, min_y, P, Q, pixels=pix)
        _check(gpu[:, pix], ref, clear, what="brute")
    assert np.isfinite(gpu).mean() > 0.05 and (~np.isfinite(gpu)).any()


# ---------------------------------------------------------------------------------------------------------- (b) pyramid edges
def test_spikes_on_pyramid_block_boundaries():
    """Flat ground with single-node spikes on nodes shared by two or four 8- and 64-cell blocks, on the last row and column
    (partial blocks) and at node (0, 0); cameras 1-2 m up look at each spike from the four directions."""
    H, W, res, x0, y0 = 150, 139, 0.05, -2.5, 1.0
    spikes = [(0, 0, 1.5), (8, 16, 1.0), (64, 64, 3.0), (64, 30, 2.0), (40, 64, 1.2), (128, 128, 2.5), (H - 1, 70, 1.8),
              (77, W - 1, 2.2), (H - 1, W - 1, 1.1), (16, 128, 1.4)]
    height = np.zeros((H, W), np.float32)
    for i, j, z in spikes:
        height[i, j] = z
    cam = CameraCfg(width=48, height=36, focal_length=12.0)        # a narrow lens: a spike's slopes are a few pixels wide
    pos, quat = [], []
    for i, j, z in spikes:
        sx, sy = x0 + j * res, y0 + i * res
        down = math.atan2(1.5 - 0.5 * z, 1.3)                          # the optical axis on the spike's middle (mount: 40 deg down)
        for yaw in (0.0, 0.5 * math.pi, math.pi, -0.5 * math.pi):
            pos.append((sx - 1.3 * math.cos(yaw), sy - 1.3 * math.sin(yaw), 1.5 - 0.73428))
            quat.append(_quat(yaw, down - math.radians(40.0), 0.0))
    n = len(pos)
    rig = Rig(n)
    rig.bind(height, res, x0, y0)
    P, Q = rig.set_poses(pos, quat)
    gpu = rig.render(cam).reshape(n, -1)
    rig.close()
    ref, clear = _reference(cam, height, res, x0, y0, P, Q, brute=False)
    _check(gpu, ref, clear, share=0, what="cast")
    # the pixels that see a spike's slopes, against the brute-force mesh
    o, d = camera_rays(cam, P, Q)
    hit = o[:, None, :] + np.where(np.isfinite(ref), ref, 0.0)[..., None] * d.reshape(n, -1, 3)
    on_spike = np.isfinite(ref) & (hit[..., 2] > 1e-6)
    assert on_spike.sum(1).min() > 0, "a camera does not see its spike"
    rows, cols = np.nonzero(on_spike)
    pick = np.random.default_rng(2).permutation(rows.size)[:3000]
    rows, cols = rows[pick], cols[pick]
    org, dirs = o[rows], d.reshape(n, -1, 3)[rows, cols]
    brute = cast_brute(height, res, x0, y0, org, dirs, cam.near_clip, cam.far_clip)
    _check(gpu[rows, cols], brute, clear[rows, cols], share=0, what="brute")


# ---------------------------------------------------------------------------------------------------------- (c) camera configs
@pytest.fixture(scope="module")
def rough_small():
    H, W, res, x0, y0 = 120, 101, 0.05, -1.2, 0.6
    return _rough((H, W), seed=5), res, x0, y0


def _rough_poses(height, res, x0, y0, n, seed, above=(0.1, 0.5)):
    H, W = height.shape
    rng = np.random.default_rng(seed)
    x = x0 + rng.uniform(0.15, 0.85, n) * (W - 1) * res
    y = y0 + rng.uniform(0.15, 0.85, n) * (H - 1) * res
    z = _surface(height, res, x0, y0, x, y) + rng.uniform(*above, n)
    quat = [_quat(rng.uniform(-math.pi, math.pi), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)) for _ in range(n)]
    return np.stack([x, y, z], 1), quat


@pytest.mark.parametrize("kw,brute", [({"width": 1, "height": 1}, True), ({"width": 7, "height": 5}, True), ({"width": 8, "height": 8}, True),
                                      ({"width": 37, "height": 23}, True), ({"width": 320, "height": 180}, False),
                                      ({"vertical_aperture": 2.968879962}, False),
                                      ({"width": 80, "height": 45, "near_clip": 0.5}, True),
                                      ({"width": 80, "height": 45, "near_clip": 2.0}, True),
                                      ({"width": 80, "height": 45, "far_clip": 3.0}, True)])
def test_camera_configs(rough_small, kw, brute):
    height, res, x0, y0 = rough_small
    cam = CameraCfg(**kw)
    n = 4
    # near_clip 0.5 matters only for a camera close to the ground: lower the bodies so that it hangs 0.15 - 0.45 m up
    pos, quat = _rough_poses(height, res, x0, y0, n, seed=6, above=(-0.6, -0.3) if cam.near_clip == 0.5 else (0.1, 0.5))
    if cam.width * cam.height <= 8:      # a pixel or two per env: many poses, looking down
        n = 64
        pos, quat = _rough_poses(height, res, x0, y0, n, seed=3)
        quat = [_quat(y, 0.5, 0.0) for y in np.linspace(-math.pi, math.pi, n)]
    rig = Rig(n)
    rig.bind(height, res, x0, y0)
    P, Q = rig.set_poses(pos, quat)
    gpu = rig.render(cam).reshape(n, -1)
    rig.close()
    if brute:
        ref, clear = _reference(cam, height, res, x0, y0, P, Q)
        _check(gpu, ref, clear, what="brute")
    else:
        ref, clear = _reference(cam, height, res, x0, y0, P, Q, brute=False)
        _check(gpu, ref, clear, what="cast")
        pix = np.random.default_rng(4).choice(gpu.shape[1], 500, replace=False)
        ref_b, clear_b = _reference(cam, height, res, x0, y0, P, Q, pixels=pix)
        _check(gpu[:, pix], ref_b, clear_b, what="brute")
    fin = np.isfinite(gpu)
    assert fin.any() and (gpu[fin] >= cam.near_clip).all() and (gpu[fin] <= cam.far_clip).all()
    if cam.near_clip > 0.1 or cam.far_clip < 1e6:     # the clip range removes hits the unclipped camera has
        free = CameraCfg(**{**kw, "near_clip": 0.01, "far_clip": 1e6})
        ref_free, _ = _reference(free, height, res, x0, y0, P, Q, brute=False)
        assert (np.isfinite(ref_free) & ~fin).sum() > 0.01 * fin.size


def test_scaled_mount_quaternion_renders_bit_identical_images(rough_small):
    """The library normalises the mount quaternion: 4 q (an exact power-of-two scale) gives the image of q, bit for bit."""
    height, res, x0, y0 = rough_small
    n = 8
    pos, quat = _rough_poses(height, res, x0, y0, n, seed=8)
    rig = Rig(n)
    rig.bind(height, res, x0, y0)
    rig.set_poses(pos, quat)
    q = np.float32(CameraCfg().orientation)                 # the reference's quaternion, |q|^2 = 1.0000138
    for q in (q, np.float32(q / np.linalg.norm(np.float64(q)))):
        a = rig.render(CameraCfg(orientation=tuple(float(c) for c in q)))
        b = rig.render(CameraCfg(orientation=tuple(float(4 * c) for c in q)))       # exact in fp32
        assert np.isfinite(a).mean() > 0.3
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    rig.close()


# ---------------------------------------------------------------------------------------------------------- (d) axis-aligned rays
def _mount(look):
    """A mount quaternion with components in {0, +-0.5, +-1} (an exact rotation matrix of 0 and +-1) whose optical axis is
    ``look`` in the Body frame."""
    from camera_reference import quat_to_mat
    cands = [(1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0)]
    cands += [tuple(0.5 * s for s in (a, b, c, e)) for a in (1, -1) for b in (1, -1) for c in (1, -1) for e in (1, -1)]
    for q in cands:
        R = quat_to_mat(q)
        if np.array_equal(R @ [0.0, 0.0, -1.0], np.asarray(look, np.float64)):
            return q
    raise AssertionError(look)


@pytest.fixture(scope="module")
def axis_terrain():
    H, W, res, x0, y0 = 61, 47, 0.05, 0.3, -1.1
    return _rough((H, W), seed=9), res, x0, y0


@pytest.mark.parametrize("look", [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0)])
def test_horizontal_rays(axis_terrain, look):
    """Identity body, a mount looking along a grid axis: the centre row or column has dz = 0 exactly (and the centre pixel two
    zero components); the camera below, at and above the terrain's maximum height."""
    height, res, x0, y0 = axis_terrain
    H, W = height.shape
    cam = CameraCfg(width=15, height=11, position=(0.0, 0.0, 0.0), orientation=_mount(look))
    top = float(height.max())
    rng = np.random.default_rng(10)
    pos = []
    for z in (top + 0.2, top, top - 0.15, float(np.median(height)), float(height.min()) - 0.05):
        for _ in range(3):
            pos.append((x0 + rng.uniform(0.2, 0.8) * (W - 1) * res, y0 + rng.uniform(0.2, 0.8) * (H - 1) * res, z))
    n = len(pos)
    quat = [(1.0, 0.0, 0.0, 0.0)] * n
    rig = Rig(n)
    rig.bind(height, res, x0, y0)
    P, Q = rig.set_poses(pos, quat)
    gpu = rig.render(cam)
    rig.close()
    o, d = camera_rays(cam, P, Q)
    level, up = d[..., 2] == 0, d[..., 2] > 0
    assert (level[:, 5, :].all() or level[:, :, 7].all()) and (d[:, 5, 7] == 0).sum(-1).min() == 2   # exactly axis-aligned
    ref, clear = _reference(cam, height, res, x0, y0, P, Q)
    _check(gpu.reshape(n, -1), ref, clear, share=0, what="brute")
    assert np.isinf(gpu[:3][level[:3] | up[:3]]).all()     # above the maximum, level or climbing: nothing to hit
    assert np.isfinite(gpu[6:12][level[6:12]]).any()       # below it the level rays meet the relief


def test_rays_along_the_grid_axes_and_vertical(axis_terrain):
    """Identity body and mounts looking straight down (centre column dx = 0, centre row dy = 0, centre pixel dx = dy = 0) and
    straight up from below the surface; the vertical centre pixel equals the height scanner's oracle."""
    height, res, x0, y0 = axis_terrain
    H, W = height.shape
    rng = np.random.default_rng(11)
    n = 12
    x = x0 + rng.uniform(0.1, 0.9, n) * (W - 1) * res
    y = y0 + rng.uniform(0.1, 0.9, n) * (H - 1) * res
    x[:2] = x0 + 7 * res, x0 + (W - 1.5) * res          # on a node column, in the last column of cells
    y[:2] = y0 + 11 * res, y0 + 3 * res
    surf = _surface(height, res, x0, y0, x, y)
    top = float(height.max())
    rig = Rig(n)
    rig.bind(height, res, x0, y0)
    quat = [(1.0, 0.0, 0.0, 0.0)] * n
    V, F = heightfield_mesh(np.asarray(height, np.float64), res, x0, y0)
    for look, z in (((0, 0, -1), np.where(np.arange(n) % 2 == 0, top + 1.5, surf + 0.4)), ((0, 0, 1), surf - 0.3)):
        cam = CameraCfg(width=9, height=7, position=(0.0, 0.0, 0.0), orientation=_mount(look))
        P, Q = rig.set_poses(np.stack([x, y, z], 1), quat)
        gpu = rig.render(cam)
        o, d = camera_rays(cam, P, Q)
        assert (d[:, :, 4, 0] == 0).all() and (d[:, 3, :, 1] == 0).all() and (d[:, 3, 4, :2] == 0).all()
        ref, clear = _reference(cam, height, res, x0, y0, P, Q)
        _check(gpu.reshape(n, -1), ref, clear, share=0, what=f"brute, looking {look}")
        scan = vertical_ray_hits(V, F, P[:, :2])
        want = P[:, 2] - scan if look[2] < 0 else scan - P[:, 2]
        assert np.isfinite(want).all()
        assert np.allclose(gpu[:, 3, 4], want, rtol=1e-5, atol=1e-5), (gpu[:, 3, 4], want)
    rig.close()


# ---------------------------------------------------------------------------------------------------------- (e) poses
def test_poses_outside_above_below_and_upside_down(rough_small):
    height, res, x0, y0 = rough_small
    H, W = height.shape
    x1, y1 = x0 + (W - 1) * res, y0 + (H - 1) * res
    xm, ym = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
    top = float(height.max())
    lift = 0.73428
    poses = [((x0 - 1.0, ym, top + 0.6 - lift), _quat(0.0, 0.0, 0.0)),                   # outside, each side, looking in
             ((x1 + 1.0, ym, top + 0.6 - lift), _quat(math.pi, 0.0, 0.0)),
             ((xm, y0 - 1.0, top + 0.6 - lift), _quat(0.5 * math.pi, 0.0, 0.0)),
             ((xm, y1 + 1.0, top + 0.6 - lift), _quat(-0.5 * math.pi, 0.0, 0.0)),
             ((x0 - 0.8, y0 - 0.6, top + 1.0 - lift), _quat(0.25 * math.pi, 0.1, 0.0)),    # a corner
             ((x1 + 0.5, y1 + 0.5, top + 0.2 - lift), _quat(-0.75 * math.pi, -0.1, 0.0)),
             ((xm, ym, top + 6.0), _quat(0.3, 0.75, 0.0)),                                 # high above, steeply down
             ((xm + 0.5, ym - 0.4, top + 3.0), _quat(2.0, 0.6, 0.2)),
             ((xm - 0.3, ym + 0.2, 0.0), _quat(0.7, -0.3, 0.0)),                            # buried (z set below)
             ((xm + 0.2, ym - 0.6, 0.0), _quat(-2.2, -0.8, 0.1)),
             ((xm - 0.7, ym, 0.0), _quat(1.0, 1.3, math.pi)),                              # upside down (z set below),
             ((xm + 0.8, ym + 0.5, 0.0), _quat(-0.4, 1.0, math.pi))]                       # nosed down to see the ground
    pos = np.array([p for p, _ in poses])
    quat = [q for _, q in poses]
    surf = _surface(height, res, x0, y0, pos[8:, 0], pos[8:, 1])
    pos[8:10, 2] = surf[:2] - 1.2                 # the camera 0.47 m under the surface
    pos[10:, 2] = surf[2:] + 1.3                  # upside down: the camera hangs 0.57 m above the surface
    n = len(poses)
    cam = CameraCfg(width=48, height=27)
    rig = Rig(n)
    rig.bind(height, res, x0, y0)
    P, Q = rig.set_poses(pos, quat)
    gpu = rig.render(cam).reshape(n, -1)
    rig.close()
    ref, clear = _reference(cam, height, res, x0, y0, P, Q)
    _check(gpu, ref, clear, share=0, what="brute")
    hits = np.isfinite(gpu).mean(1)
    assert (hits > 0.1).all(), hits


def test_plateau_at_the_maximum_seen_from_above():
    """A mesa whose flat top is the terrain's maximum, seen from 2 - 4 m above: most rays enter their range exactly on the
    surface (the from_top path), where the gap at the entry may round a hair below zero and only the entry rule says "above"."""
    H, W, res, x0, y0 = 90, 77, 0.05, -0.8, -2.1
    rough = _rough((H, W), seed=15)
    height = np.minimum(rough, np.float32(np.quantile(rough, 0.3)))
    top = float(height.max())
    rng = np.random.default_rng(16)
    n = 12
    pos = np.stack([x0 + rng.uniform(0.3, 0.7, n) * (W - 1) * res, y0 + rng.uniform(0.3, 0.7, n) * (H - 1) * res,
                    top + rng.uniform(2.0, 4.0, n)], 1)
    quat = [_quat(rng.uniform(-math.pi, math.pi), rng.uniform(0.6, 0.9), rng.uniform(-0.1, 0.1)) for _ in range(n)]
    cam = CameraCfg(width=48, height=27, focal_length=12.0)
    rig = Rig(n)
    rig.bind(height, res, x0, y0)
    P, Q = rig.set_poses(pos, quat)
    gpu = rig.render(cam).reshape(n, -1)
    rig.close()
    ref, clear = _reference(cam, height, res, x0, y0, P, Q)
    _check(gpu, ref, clear, share=0, what="brute")
    o, d = camera_rays(cam, P, Q)
    z_hit = o[:, None, 2] + ref * d.reshape(n, -1, 3)[..., 2]
    assert (np.abs(z_hit - top) < 1e-9).mean() > 0.3          # most pixels see the top of the mesa


# ---------------------------------------------------------------------------------------------------------- (f) degenerate states
def test_degenerate_states_render_inf_and_leave_the_others_alone(rough_small):
    height, res, x0, y0 = rough_small
    n = 10
    pos, quat = _rough_poses(height, res, x0, y0, n, seed=12)
    quat = np.array(quat)
    cam = CameraCfg(width=37, height=23)
    rig = Rig(n)
    rig.bind(height, res, x0, y0)
    rig.set_poses(pos, quat)
    clean = rig.render(cam)
    bad_pos, bad_quat = pos.copy(), quat.copy()
    bad_pos[1, 0] = np.nan
    bad_pos[3, 2] = np.nan
    bad_quat[4] = 0.0
    bad_pos[6] = (1e6, 2.0, 0.5)
    bad_pos[8] = (x0 + 1.0, -1e6, 0.5)
    rig.set_poses(bad_pos, bad_quat)
    dirty = rig.render(cam)
    rig.close()
    bad = [1, 3, 4, 6, 8]
    good = [k for k in range(n) if k not in bad]
    assert np.isposinf(dirty[bad]).all()
    assert np.isfinite(clean[good]).mean() > 0.3
    assert np.array_equal(dirty[good].view(np.uint32), clean[good].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------- (g) bench workload
def test_bench_workload_matches_the_reference():
    """tools/camera_bench.py's workload: config-2 terrain (2048^2, seed 1234, 400 rocks), 4096 envs, the states of its 300-step
    pre-roll of random actions; 8 sampled envs against cast."""
    n = 4096
    ter = T.make_procedural_terrain((2048, 2048), seed=1234, sigma_z=0.15, n_rocks=400)
    ter.make_spawns(2 * n)
    env = _env(ter, n, CameraCfg())
    g = torch.Generator(device=DEV).manual_seed(0)
    env.reset()
    for _ in range(300):
        env.step(torch.rand(n, 2, device=DEV, generator=g) * 2 - 1)
    depth = env.extras["depth"].permute(0, 2, 1)
    assert torch.equal(depth, env.render_depth().permute(0, 2, 1))
    pick = np.random.default_rng(13).choice(n, 8, replace=False)
    S = env.get_state().cpu().numpy()[pick]
    gpu = depth[torch.as_tensor(pick, device=DEV)].cpu().numpy().reshape(8, -1)
    env.close()
    cam = CameraCfg()
    ref, clear = _reference(cam, ter.height, ter.resolution, ter.min_x, ter.min_y, S[:, _lib.POS:_lib.POS + 3].astype(np.float64),
                            S[:, _lib.QUAT:_lib.QUAT + 4].astype(np.float64), brute=False)
    _check(gpu, ref, clear, what="cast")
    assert np.isfinite(gpu).mean() > 0.5


# ---------------------------------------------------------------------------------------------------------- (h) past 2^31 elements
def test_output_past_two_to_the_31_elements():
    """2050 envs x 1024 x 1024 pixels in one buffer (8.6 GB): env 2048 starts at element 2^31 exactly."""
    n, side = 2050, 1024
    assert 2048 * side * side == 2 ** 31
    ter = T.make_procedural_terrain((512, 512), seed=21, n_rocks=40)
    ter.make_spawns(2 * 2048, border_offset=2.0)
    env = _env(ter, n)
    env.reset()
    lib, h = env._lib, env._h
    cam = CameraCfg(width=side, height=side)
    cfg = cam.to_native()
    nb = int(lib.rover_camera_workspace_bytes(h, C.byref(cfg)))
    ws = torch.zeros((nb + 3) // 4, dtype=torch.float32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    assert lib.rover_camera_prepare(h, C.byref(cfg), _ptr(ws), nb, st) == 0
    S = env.get_state().clone()
    sel = [0, 2047, 2048, 2049]
    res = ter.resolution
    for k, e in enumerate(sel):
        x, y = ter.min_x + (100 + 90 * k) * res, ter.min_y + (140 + 70 * k) * res
        S[e, _lib.POS:_lib.POS + 3] = torch.tensor([x, y, float(ter.height[140 + 70 * k, 100 + 90 * k]) + 0.2 + 0.1 * k])
        S[e, _lib.QUAT:_lib.QUAT + 4] = torch.tensor(_quat(0.5 + 1.6 * k, 0.1 * k, -0.05 * k), dtype=torch.float32)
    env.set_state(S)
    buf = torch.full((n, side, side), float("nan"), dtype=torch.float32, device=DEV)
    assert lib.rover_camera_render(h, C.byref(cfg), _ptr(ws), _ptr(buf), st) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(buf).any())
    gpu = buf[torch.as_tensor(sel, device=DEV)].cpu().numpy().reshape(len(sel), -1)
    del buf
    Sn = env.get_state().cpu().numpy()[sel]
    env.close()
    torch.cuda.empty_cache()
    pix = np.random.default_rng(14).choice(side * side, 4000, replace=False)
    ref, clear = _reference(cam, ter.height, res, ter.min_x, ter.min_y, Sn[:, _lib.POS:_lib.POS + 3].astype(np.float64),
                            Sn[:, _lib.QUAT:_lib.QUAT + 4].astype(np.float64), brute=False, pixels=pix)
    _check(gpu[:, pix], ref, clear, what="cast")
    assert np.isfinite(gpu[:, pix]).mean(1).min() > 0.2


# ---------------------------------------------------------------------------------------------------------- (i) refusals
def test_render_between_step_begin_and_finish_is_refused():
    n = 64
    ter = _flat_terrain()
    env = _env(ter, n, CameraCfg())
    env.reset()
    lib, h = env._lib, env._h
    cfg, ws = env.sensors.camera_cfg, _ptr(env.sensors.workspace)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    buf = torch.empty(n, 90, 160, device=DEV)
    a = torch.zeros(n, 2, device=DEV)
    obs = torch.zeros(n, env.obs_dim, device=DEV)
    rew = torch.zeros(n, device=DEV)
    flags = torch.zeros(2, n, dtype=torch.uint8, device=DEV)
    force = torch.zeros(39, n, device=DEV)
    log = torch.zeros(16, device=DEV)
    assert lib.rover_step_begin(h, _ptr(a), _ptr(rew), _ptr(flags[0]), _ptr(flags[1]), _ptr(force), st) == 0
    assert lib.rover_camera_render(h, C.byref(cfg), ws, _ptr(buf), st) == ERR_STATE
    assert b"between rover_step_begin and rover_step_finish" in lib.rover_last_error()
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    assert lib.rover_step_finish(h, _ptr(mask), _ptr(obs), _ptr(force), _ptr(log), st) == 0
    assert lib.rover_camera_render(h, C.byref(cfg), ws, _ptr(buf), st) == 0
    # a workspace other than the prepared one
    other = torch.zeros_like(env.sensors.workspace)
    assert lib.rover_camera_render(h, C.byref(cfg), _ptr(other), _ptr(buf), st) == ERR_STATE
    assert b"prepare" in lib.rover_last_error()
    torch.cuda.synchronize()
    env.close()


_BAD = [("focal_length", math.inf), ("focal_length", math.nan), ("focal_length", 0.0), ("horizontal_aperture", math.inf),
        ("horizontal_aperture", math.nan), ("vertical_aperture", math.inf), ("vertical_aperture", math.nan),
        ("mount_pos", (0.0, math.nan, 0.5)), ("mount_pos", (math.inf, 0.0, 0.5)), ("mount_quat", (math.nan, 0.0, 0.0, 1.0)),
        ("mount_quat", (1.0, 0.0, -math.inf, 0.0)), ("mount_quat", (0.0, 0.0, 0.0, 0.0)), ("near_clip", math.nan),
        ("far_clip", math.nan), ("near_clip", -0.5), ("width", 0), ("height", -3)]
_CFG_NAME = {"mount_pos": "position", "mount_quat": "orientation"}


def test_invalid_configs_are_refused_by_the_library_and_the_cfg():
    env = _env(_flat_terrain(), 8, CameraCfg())
    env.reset()
    lib, h = env._lib, env._h
    nb = int(env.sensors.workspace.numel() * 4)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    buf = torch.empty(8, 90, 160, device=DEV)
    for field, value in _BAD:
        cfg = CameraCfg().to_native()
        if isinstance(value, tuple):
            for i, v in enumerate(value):
                getattr(cfg, field)[i] = v
        else:
            setattr(cfg, field, value)
        assert lib.rover_camera_workspace_bytes(h, C.byref(cfg)) == 0, field
        assert lib.rover_camera_prepare(h, C.byref(cfg), _ptr(env.sensors.workspace), nb, st) == ERR_INVALID, (field, value)
        assert lib.rover_camera_render(h, C.byref(cfg), _ptr(env.sensors.workspace), _ptr(buf), st) == ERR_INVALID, (field, value)
        cam = CameraCfg()
        setattr(cam, _CFG_NAME.get(field, field), value)
        with pytest.raises(ValueError):
            cam.validate()
    ok = CameraCfg(far_clip=math.inf).to_native()              # an infinite far clip stays allowed
    assert lib.rover_camera_workspace_bytes(h, C.byref(ok)) == nb
    torch.cuda.synchronize()
    env.close()


# ---------------------------------------------------------------------------------------------------------- device guard
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_camera_env_on_second_device_while_first_is_current():
    """rover_camera_prepare / rover_camera_render run on the handle's device whatever the thread's current device is."""
    ter = T.make_procedural_terrain((512, 512), seed=21, n_rocks=40)
    ter.make_spawns(2 * 64, border_offset=2.0)
    torch.cuda.set_device(0)
    envs = [_env(ter, 64, CameraCfg(), device=dev) for dev in ("cuda:0", "cuda:1")]
    torch.cuda.set_device(0)
    outs = []
    for e in envs:
        _, extras = e.reset()
        outs.append(extras["depth"].cpu())
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).any()
    a = torch.rand(64, 2, generator=torch.Generator().manual_seed(1)) * 2 - 1
    for _ in range(3):
        outs = [e.step(a.to(e.device))[4]["depth"].cpu() for e in envs]
        assert torch.equal(outs[0], outs[1])
    assert torch.equal(envs[1].render_depth().cpu(), outs[1])
    for e in envs:
        e.close()
