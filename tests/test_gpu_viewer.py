"""rgb_array viewer on the MI355X: RoverEnv.render(), the HIP render against the float64 reference renderer (viewer_reference.py)
on small terrains with posed rovers, the march-skip hazard, the map's edge, the C entry's refusals, that rendering changes nothing
in the simulation, the bench-scale frames, and RecordVideo through the compat registry.

Comparison rule (kernel vs reference, per pixel):
  * object_id equal, except where the reference marks the pixel ambiguous: its two nearest hits (of different objects) lie within
    EPS_T = 1e-4 (1 + depth) metres, or its id changes when every rover part and target grows or shrinks by 1e-4 m (a silhouette);
    the ambiguous count is reported and must stay under 2 % of the frame, and at most 0.05 % of the pixels may disagree otherwise;
  * where the ids agree: RGB within 1 LSB and depth within 1e-4 relative + 1e-4 m, allowing 0.1 % of the pixels (a hit on a
    triangle's edge may be shaded with its neighbour's normal).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import viewer_reference as vr
from isaac_rover_orbit_amd import _lib
from isaac_rover_orbit_amd import terrain as T
from isaac_rover_orbit_amd.cfg import RoverEnvCfg, ViewerCfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS_T = 1e-4


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _terrain(kind, shape=(160, 160), min_x=0.0, min_y=0.0, seed=3):
    H, W = shape
    rng = np.random.RandomState(seed)
    if kind == "flat":
        g = np.zeros(shape, np.float32)
    elif kind == "random":
        g = (0.08 * rng.standard_normal(shape)).astype(np.float32)
    elif kind == "checker":
        i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        g = np.where(((i // 4) + (j // 4)) % 2 == 0, 0.15, 0.0).astype(np.float32)
    ob = np.zeros(shape, np.float32)
    if kind in ("random", "rocks"):
        if kind == "rocks":
            g = (0.03 * rng.standard_normal(shape)).astype(np.float32)
        for _ in range(6):
            ci, cj, r = rng.randint(10, H - 10), rng.randint(10, W - 10), rng.randint(3, 8)
            i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            bump = np.maximum(0.0, 0.4 * (1 - ((i - ci) ** 2 + (j - cj) ** 2) / r ** 2)).astype(np.float32)
            ob = np.maximum(ob, bump)
    zero = np.zeros(shape, np.uint8)
    ter = T.Terrain(ground=g, obstacle=ob, min_x=min_x, min_y=min_y, rock_mask=zero, safe_rock_mask=zero.copy())
    sp = np.zeros((64, 3), np.float32)
    sp[:, 0], sp[:, 1] = min_x + 0.5 * W * T.RESOLUTION, min_y + 0.5 * H * T.RESOLUTION
    ter.spawn_locations = sp
    return ter


def _env(ter, n, render_mode="rgb_array", viewer=None, **kw):
    from isaac_rover_orbit_amd.envs import RoverEnv
    cfg = RoverEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.terrain.kind = "custom"
    if viewer is not None:
        cfg.viewer = viewer
    for k, v in kw.items():
        setattr(cfg, k, v)
    return RoverEnv(cfg, terrain=ter, render_mode=render_mode)


def _quat(yaw, pitch=0.0, roll=0.0):
    cy, sy, cp, sp, cr, sr = (math.cos(yaw / 2), math.sin(yaw / 2), math.cos(pitch / 2), math.sin(pitch / 2),
                              math.cos(roll / 2), math.sin(roll / 2))
    return [cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy]


def _pose(env, rows):
    """rows: per env (x, y, z, yaw, pitch, roll, bogie (3), steer (4), target (x, y, z)); returns the state as set (float32)."""
    S = env.get_state().clone()
    for e, r in enumerate(rows):
        x, y, z, yaw, pitch, roll, bq, sq, tg = r
        S[e, _lib.POS:_lib.POS + 3] = torch.tensor([x, y, z])
        S[e, _lib.QUAT:_lib.QUAT + 4] = torch.tensor(_quat(yaw, pitch, roll))
        S[e, _lib.BOGIE_Q:_lib.BOGIE_Q + 3] = torch.tensor(bq)
        S[e, _lib.STEER_Q:_lib.STEER_Q + 4] = torch.tensor(sq)
        S[e, _lib.TARGET_W:_lib.TARGET_W + 3] = torch.tensor(tg)
    env.set_state(S)
    return env.get_state().cpu().numpy()


def _compare(env, ter, viewer, state=None, what=""):
    env.cfg.viewer = viewer
    rgba, dep, ids = env.render_frame(depth=True, object_id=True)
    torch.cuda.synchronize()
    rgba, dep, ids = rgba.cpu().numpy(), dep.cpu().numpy(), ids.cpu().numpy()
    S = env.get_state().cpu().numpy() if state is None else state
    rgb_r, dep_r, id_r, gap, graze = vr.render(viewer, ter.height, ter.obstacle, ter.resolution, ter.min_x, ter.min_y, S)
    npx = ids.size
    amb = (gap < EPS_T * (1 + np.where(np.isfinite(dep_r), dep_r, 0))) | graze
    diff = ids != id_r
    unexplained = diff & ~amb
    assert amb.sum() < 0.02 * npx, f"{what}: {amb.sum()} ambiguous pixels"
    assert unexplained.sum() <= max(1, int(5e-4 * npx)), f"{what}: {unexplained.sum()} id mismatches outside the ambiguous set " \
        f"{list(zip(*np.nonzero(unexplained)))[:5]} gpu {ids[unexplained][:5]} ref {id_r[unexplained][:5]}"
    same = ~diff
    drgb = np.abs(rgba[..., :3].astype(int) - rgb_r.astype(int)).max(-1)
    bad_rgb = same & (drgb > 1)
    fin = same & np.isfinite(dep_r)
    assert (np.isinf(dep[same & ~np.isfinite(dep_r)])).all()
    bad_dep = np.zeros_like(same)
    bad_dep[fin] = np.abs(dep[fin] - dep_r[fin]) > 1e-4 * dep_r[fin] + 1e-4
    assert bad_rgb.sum() <= max(1, int(1e-3 * npx)), f"{what}: {bad_rgb.sum()} pixels off by > 1 LSB"
    assert bad_dep.sum() <= max(1, int(1e-3 * npx)), f"{what}: {bad_dep.sum()} depths out of tolerance"
    assert (rgba[..., 3] == 255).all()
    print(f"{what}: ambiguous {int(amb.sum())}, id mismatches {int(diff.sum())} ({int(unexplained.sum())} unexplained), "
          f"rgb > 1 LSB {int(bad_rgb.sum())}, depth {int(bad_dep.sum())} of {npx}")
    return ids, id_r


def test_render_returns_the_rgb_array_frame():
    ter = _terrain("random")
    env = _env(ter, 4)
    assert env.render_mode == "rgb_array" and "rgb_array" in env.metadata["render_modes"]
    env.reset()
    img = env.render()
    assert isinstance(img, np.ndarray) and img.shape == (720, 1280, 3) and img.dtype == np.uint8
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 10
    dev = env.render_rgb()
    assert dev.shape == (720, 1280, 4) and dev.dtype == torch.uint8 and dev.device.type == "cuda"
    env.close()
    off = _env(ter, 4, render_mode=None)
    off.reset()
    assert off.render() is None
    off.close()
    from isaac_rover_orbit_amd.envs import RoverEnv
    vp = RoverEnv(off.cfg, terrain=ter, viewport=True)                 # what the reference passes for --video
    assert vp.render_mode == "rgb_array"
    vp.close()


ROWS = [  # x, y, z, yaw, pitch, roll, bogie, steer, target
    (2.0, 2.0, 0.30, 0.3, 0.0, 0.0, [0, 0, 0], [0, 0, 0, 0], [3.0, 5.5, 0.0]),
    (4.5, 3.0, 0.35, 2.0, 0.15, -0.1, [0.17, -0.1, 0.05], [0.6, -0.4, 0.3, -0.7], [6.0, 1.5, 0.1]),
    (3.0, 5.0, 0.40, -1.2, -0.2, 0.25, [-0.15, 0.12, -0.17], [1.2, 1.0, -1.1, 0.2], [1.0, 6.5, 0.0]),
    (6.0, 6.0, 0.30, 0.9, 0.05, 0.3, [0.05, 0.05, 0.1], [-0.3, 0.3, 0.8, -0.8], [5.0, 7.0, 0.2]),
]
VIEWS = [ViewerCfg(eye=(-1.5, -1.0, 3.0), lookat=(4.0, 4.0, 0.0), resolution=(160, 90)),
         ViewerCfg(eye=(9.0, 3.0, 1.2), lookat=(3.0, 4.0, 0.2), resolution=(320, 180)),
         ViewerCfg(eye=(-6.0, -6.0, 3.5), lookat=(0.0, 0.0, 0.0), resolution=(160, 90))]      # the reference's world-origin view


@pytest.mark.parametrize("kind", ["random", "checker", "rocks"])
def test_kernel_matches_reference_on_posed_rovers(kind):
    ter = _terrain(kind)
    env = _env(ter, 4)
    env.reset()
    S = _pose(env, ROWS)
    for i, v in enumerate(VIEWS):
        ids, _ = _compare(env, ter, v, S, f"{kind} view {i}")
        if i < 2:
            assert (ids >= vr.ID_ENV0).sum() > 100          # rovers are in the picture
    env.close()


def test_kernel_matches_reference_after_steps_and_env_origin():
    ter = _terrain("rocks", shape=(256, 256))
    env = _env(ter, 6)
    env.reset()
    g = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(30):
        env.step(torch.rand(6, 2, device=DEV, generator=g) * 2 - 1)
    v = ViewerCfg(eye=(-2.5, -2.0, 1.5), lookat=(0.0, 0.0, 0.2), resolution=(160, 90), origin_type="env", env_index=2)
    ids, _ = _compare(env, ter, v, what="after steps, env origin")
    assert ((ids - vr.ID_ENV0) // vr.IDS_PER_ENV == 2).sum() > 200       # env 2 is what the camera follows
    env.close()


def test_rover_on_a_block_the_terrain_skip_skips():
    """Flat terrain and a grazing view: the terrain march skips every 64-cell block the ray crosses above z = 0, including the
    one a rover stands on -- the rover must still be drawn."""
    ter = _terrain("flat", shape=(400, 400))
    env = _env(ter, 2)
    env.reset()
    S = _pose(env, [(12.0, 12.0, 0.27, 0.5, 0, 0, [0, 0, 0], [0, 0, 0, 0], [15.0, 12.0, 0.0]),
                    (16.0, 5.0, 0.27, 0.0, 0, 0, [0, 0, 0], [0, 0, 0, 0], [16.0, 9.0, 0.0])])
    v = ViewerCfg(eye=(1.0, 1.0, 0.6), lookat=(12.0, 12.0, 0.2), resolution=(160, 90))
    ids, id_r = _compare(env, ter, v, S, "grazing view over flat terrain")
    env0 = lambda x: (x >= vr.ID_ENV0) & (x < vr.ID_ENV0 + 7)        # noqa: E731  (env 0's chassis and wheels)
    assert env0(id_r).sum() > 20 and env0(ids).sum() > 20
    env.close()


def test_rover_half_off_the_edge_is_drawn():
    ter = _terrain("random")
    env = _env(ter, 2)
    env.reset()
    S = _pose(env, [(-0.1, 4.0, 0.3, 0.0, 0, 0, [0, 0, 0], [0, 0, 0, 0], [-0.5, 6.0, 0.0]),
                    (4.0, 8.2, 0.3, 1.5, 0, 0, [0, 0, 0], [0, 0, 0, 0], [2.0, 2.0, 0.0])])
    v = ViewerCfg(eye=(-4.0, 1.0, 2.0), lookat=(0.0, 5.0, 0.0), resolution=(160, 90))
    ids, _ = _compare(env, ter, v, S, "half off the edge")
    assert ((ids >= vr.ID_ENV0) & (ids < vr.ID_ENV0 + 7)).sum() > 50
    assert (ids == vr.ID_ENV0 + 7).sum() > 5                          # the target outside the map
    env.close()


def test_draw_targets_off_removes_exactly_the_targets():
    ter = _terrain("random")
    env = _env(ter, 4)
    env.reset()
    _pose(env, ROWS)
    on = ViewerCfg(eye=(-1.5, -1.0, 3.0), lookat=(4.0, 4.0, 0.0), resolution=(320, 180))
    off = ViewerCfg(eye=(-1.5, -1.0, 3.0), lookat=(4.0, 4.0, 0.0), resolution=(320, 180), draw_targets=False)
    env.cfg.viewer = on
    _, _, a = env.render_frame(object_id=True)
    env.cfg.viewer = off
    _, _, b = env.render_frame(object_id=True)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    tgt = (a >= vr.ID_ENV0) & ((a - vr.ID_ENV0) % vr.IDS_PER_ENV == 7)
    assert tgt.sum() > 20
    assert (a[~tgt] == b[~tgt]).all()
    assert not ((b >= vr.ID_ENV0) & ((b - vr.ID_ENV0) % vr.IDS_PER_ENV == 7)).any()
    env.close()


def test_refusals():
    ter = _terrain("random")
    n = 8
    env = _env(ter, n)
    env.reset()
    env.render_rgb()
    lib, h = env._lib, env._h
    ws = _ptr(env._viewer_ws)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    img = torch.empty(720, 1280, 4, dtype=torch.uint8, device=DEV)
    good = ViewerCfg().to_native(n)
    assert lib.rover_viewer_render(h, C.byref(good), ws, _ptr(img), None, None, st) == 0
    bad = []
    for f in (lambda c: c.eye.__setitem__(0, float("nan")), lambda c: c.lookat.__setitem__(2, float("inf")),
              lambda c: [c.lookat.__setitem__(i, c.eye[i]) for i in range(3)],
              lambda c: [c.lookat.__setitem__(0, c.eye[0]), c.lookat.__setitem__(1, c.eye[1])],
              lambda c: setattr(c, "width", 0), lambda c: setattr(c, "height", 8193), lambda c: setattr(c, "focal_length", 0.0),
              lambda c: setattr(c, "horizontal_aperture", float("nan")), lambda c: setattr(c, "near_clip", -1.0),
              lambda c: setattr(c, "far_clip", 0.0), lambda c: setattr(c, "origin_type", 2),
              lambda c: [setattr(c, "origin_type", 1), setattr(c, "env_index", n)],
              lambda c: [setattr(c, "origin_type", 1), setattr(c, "env_index", -1)]):
        c = ViewerCfg().to_native(n)
        f(c)
        bad.append(c)
    for c in bad:
        assert lib.rover_viewer_render(h, C.byref(c), ws, _ptr(img), None, None, st) == 1
        assert lib.rover_viewer_workspace_bytes(h, C.byref(c)) == 0
    assert lib.rover_viewer_render(h, C.byref(good), ws, None, None, None, st) == 1
    other = torch.empty_like(env._viewer_ws)
    assert lib.rover_viewer_render(h, C.byref(good), _ptr(other), _ptr(img), None, None, st) == 2
    # between rover_step_begin and rover_step_finish
    a = torch.zeros(n, 2, device=DEV)
    obs = torch.zeros(n, env.obs_dim, device=DEV)
    rew = torch.zeros(n, device=DEV)
    flags = torch.zeros(2, n, dtype=torch.uint8, device=DEV)
    force = torch.zeros(39, n, device=DEV)
    log = torch.zeros(16, device=DEV)
    assert lib.rover_step_begin(h, _ptr(a), _ptr(rew), _ptr(flags[0]), _ptr(flags[1]), _ptr(force), st) == 0
    assert lib.rover_viewer_render(h, C.byref(good), ws, _ptr(img), None, None, st) == 2
    assert b"between rover_step_begin and rover_step_finish" in lib.rover_last_error()
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    assert lib.rover_step_finish(h, _ptr(mask), _ptr(obs), _ptr(force), _ptr(log), st) == 0
    assert lib.rover_viewer_render(h, C.byref(good), ws, _ptr(img), None, None, st) == 0
    # a re-bound terrain needs a new prepare
    H, W = ter.shape
    assert lib.rover_set_terrain(h, _ptr(env._height_dev), _ptr(env._obstacle_dev), _ptr(env._mask_dev), H, W, float(ter.resolution),
                                 float(ter.min_x), float(ter.min_y), _ptr(env._spawns_dev), int(env._spawns_dev.shape[0])) == 0
    assert lib.rover_viewer_render(h, C.byref(good), ws, _ptr(img), None, None, st) == 2
    assert b"prepare" in lib.rover_last_error()
    nb = lib.rover_viewer_workspace_bytes(h, C.byref(good))
    assert lib.rover_viewer_prepare(h, C.byref(good), ws, nb, st) == 0
    assert lib.rover_viewer_render(h, C.byref(good), ws, _ptr(img), None, None, st) == 0
    torch.cuda.synchronize()
    env.close()


def test_rendering_does_not_perturb_the_simulation():
    ter = T.make_procedural_terrain((1024, 1024), seed=5, sigma_z=0.15, n_rocks=60)
    ter.make_spawns(256)
    runs = []
    for render in (True, False):
        env = _env(ter, 128, viewer=ViewerCfg(eye=(-6.0, -6.0, 3.5), resolution=(320, 180)), seed=11)
        env.reset()
        g = torch.Generator(device=DEV).manual_seed(2)
        out = []
        for _ in range(50):
            o, r, te, tr, _ = env.step(torch.rand(128, 2, device=DEV, generator=g) * 2 - 1)
            out.append((o["policy"].clone(), r.clone(), te.clone(), tr.clone()))
            if render:
                env.render()
        out.append(env.get_state().clone())
        if render:
            a, b = env.render_rgb().clone(), env.render_rgb().clone()
            assert torch.equal(a, b)                                   # the same frame twice is bit-identical
        runs.append(out)
        env.close()
    for x, y in zip(runs[0][:-1], runs[1][:-1]):
        for u, w in zip(x, y):
            assert torch.equal(u, w)
    assert torch.equal(runs[0][-1], runs[1][-1])


def test_bench_workload_frames():
    ter = T.make_procedural_terrain((2048, 2048), seed=1234, sigma_z=0.15, n_rocks=400)
    ter.make_spawns(2 * 4096, seed=41)
    env = _env(ter, 4096)
    env.reset()
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(50):
        env.step(torch.rand(4096, 2, device=DEV, generator=g) * 2 - 1)
    S = env.get_state().cpu().numpy()
    e0 = S[0, _lib.POS:_lib.POS + 3]
    for v in (ViewerCfg(eye=(-6.0, -6.0, 3.5), lookat=(0.0, 0.0, 0.0)),
              ViewerCfg(eye=tuple(e0 + [-8.0, -6.0, 4.0]), lookat=tuple(e0))):
        env.cfg.viewer = v
        rgba, dep, ids = env.render_frame(depth=True, object_id=True)
        torch.cuda.synchronize()
        rgba, dep, ids = rgba.cpu().numpy(), dep.cpu().numpy(), ids.cpu().numpy()
        rng = np.random.RandomState(0)
        rows, cols = rng.randint(0, 720, 300), rng.randint(0, 1280, 300)
        rgb_r, dep_r, id_r, gap, graze = vr.render(v, ter.height, ter.obstacle, ter.resolution, ter.min_x, ter.min_y, S,
                                                   pixels=(rows, cols))
        amb = (gap < EPS_T * (1 + np.where(np.isfinite(dep_r), dep_r, 0))) | graze
        diff = ids[rows, cols] != id_r
        assert (diff & ~amb).sum() <= 1, (diff & ~amb).sum()
        ok = ~diff
        assert (np.abs(rgba[rows, cols, :3].astype(int) - rgb_r.astype(int)).max(-1)[ok] <= 1).mean() >= 0.99
    assert (ids >= vr.ID_ENV0).sum() > 1000                            # the follow view shows rovers
    env.close()


def test_131072_envs_small_frame():
    ter = T.make_procedural_terrain((2048, 2048), seed=1234, sigma_z=0.15, n_rocks=400)
    ter.make_spawns(2 * 131072, seed=41)
    env = _env(ter, 131072, viewer=ViewerCfg(eye=(-6.0, -6.0, 20.0), lookat=(50.0, 50.0, 0.0), resolution=(320, 180)))
    env.reset()
    env.step(torch.zeros(131072, 2, device=DEV))
    _, _, ids = env.render_frame(object_id=True)
    torch.cuda.synchronize()
    assert (ids >= vr.ID_ENV0).sum().item() > 100
    env.close()


def test_record_video_through_compat(tmp_path):
    import isaac_rover_orbit_amd.compat as compat
    gym = compat.gym_api()
    compat.register_default_tasks()
    from isaac_rover_orbit_amd.cfg import AAURoverEnvCfg
    cfg = AAURoverEnvCfg()
    cfg.scene.num_envs = 16
    cfg.sim.device = DEV
    cfg.viewer = ViewerCfg(eye=(-6.0, -6.0, 3.5), resolution=(320, 180))
    env = gym.make("AAURoverEnv-v0", cfg=cfg, headless=True, viewport=True)
    assert env.unwrapped.render_mode == "rgb_array"
    folder = tmp_path / "videos"
    w = gym.wrappers.RecordVideo(env, video_folder=str(folder), step_trigger=lambda s: s == 0, video_length=10, disable_logger=True)
    w.reset()
    frames = [env.render()]
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(10):
        w.step(torch.rand(16, 2, device=DEV, generator=g) * 2 - 1)
        frames.append(env.render())
    files = sorted(os.listdir(folder))
    assert len(files) == 1 and files[0].endswith(".npz")
    rec = np.load(folder / files[0])["frames"]
    assert rec.shape == (10, 180, 320, 3) and rec.dtype == np.uint8
    assert np.array_equal(rec, np.stack(frames[:10]))
    env.close()
