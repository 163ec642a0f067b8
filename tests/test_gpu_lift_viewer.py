"""rgb_array viewer of FrankaCubeLift-v0 on the MI355X: FrankaCubeLiftEnv.render(), the HIP render against the float64 reference
renderer (lift_viewer_reference.py) on the shared posed scenes (lift_viewer_cases.py), the C entry's refusals, that rendering
changes nothing in the simulation, RecordVideo through the compat registry, and one frame at 4096 envs.

Comparison rule (kernel vs reference, per pixel) -- the rule of test_gpu_viewer.py, unchanged:
  * object_id equal, except where the reference marks the pixel ambiguous: its two nearest hits (of different objects) lie within
    EPS_T = 1e-4 (1 + depth) metres, or its id changes when every primitive grows or shrinks by 1e-4 m (a silhouette); the
    ambiguous count must stay under 2 % of the frame, and at most max(1, 0.05 %) of the pixels may disagree otherwise;
  * where the ids agree: RGB within 1 LSB and depth within 1e-4 relative + 1e-4 m, allowing 0.1 % of the pixels.
"""
import ctypes as C
import dataclasses
import math
import os
import time

import numpy as np
import pytest
import torch

import lift_viewer_cases as lc
import lift_viewer_reference as lr
from isaac_rover_orbit_amd import _lib
from isaac_rover_orbit_amd.cfg import ViewerCfg
from isaac_rover_orbit_amd.envs import lift_env as le

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS_T = 1e-4
CASES = lc.cases()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _env(n, viewer=None, spacing=2.5, render_mode="rgb_array", seed=0):
    cfg = le.LiftEnvCfg()
    cfg.scene.num_envs = n
    cfg.scene.env_spacing = spacing
    cfg.sim.device = DEV
    cfg.seed = seed
    if viewer is not None:
        cfg.viewer = viewer
    return le.FrankaCubeLiftEnv(cfg, render_mode=render_mode)


def _posed_env(case):
    env = _env(case.n, case.viewer, case.env_spacing)
    env.reset()
    if case.state is not None:
        env.set_state(torch.from_numpy(case.state))
    return env


def _frame(env):
    rgba, dep, ids = env.render_frame(depth=True, object_id=True)
    torch.cuda.synchronize()
    return rgba.cpu().numpy(), dep.cpu().numpy(), ids.cpu().numpy()


def _overflow(env):
    """Envs on the overflow list of the last render: the workspace's first int32 (include/rover_lift_viewer.h)."""
    torch.cuda.synchronize()
    return int(env._viewer_ws[:1].view(torch.int32).item())


def _compare(case):
    env = _posed_env(case)
    S = env.get_state().cpu().numpy()
    if case.state is not None:
        assert np.array_equal(S, case.state, equal_nan=True)
    rgba, dep, ids = _frame(env)
    # who the lattice walk finds: every env but one whose cube is cells away, or all of them when the cells are smaller than a table
    assert _overflow(env) == {"cube_far_away": 1, "spacing_0.5": 5}.get(case.name, 0)
    env.close()
    rgb_r, dep_r, id_r, gap, graze = lr.render(case.viewer, S, case.env_spacing, lc.EE_OFFSET_Z)
    what, npx = case.name, ids.size
    amb = (gap < EPS_T * (1 + np.where(np.isfinite(dep_r), dep_r, 0))) | graze
    diff = ids != id_r
    unexplained = diff & ~amb
    drgb = np.abs(rgba[..., :3].astype(int) - rgb_r.astype(int)).max(-1)
    same = ~diff
    bad_rgb = same & (drgb > 1)
    fin = same & np.isfinite(dep_r)
    bad_dep = np.zeros_like(same)
    bad_dep[fin] = np.abs(dep[fin] - dep_r[fin]) > 1e-4 * dep_r[fin] + 1e-4
    print(f"{what}: ambiguous {int(amb.sum())}, id mismatches {int(diff.sum())} ({int(unexplained.sum())} unexplained), "
          f"rgb > 1 LSB {int(bad_rgb.sum())}, depth {int(bad_dep.sum())} of {npx}")
    assert amb.sum() < 0.02 * npx, f"{what}: {amb.sum()} ambiguous pixels"
    assert unexplained.sum() <= max(1, int(5e-4 * npx)), f"{what}: {unexplained.sum()} id mismatches outside the ambiguous set " \
        f"{list(zip(*np.nonzero(unexplained)))[:5]} gpu {ids[unexplained][:5]} ref {id_r[unexplained][:5]}"
    assert (np.isinf(dep[same & ~np.isfinite(dep_r)])).all()
    assert bad_rgb.sum() <= max(1, int(1e-3 * npx)), f"{what}: {bad_rgb.sum()} pixels off by > 1 LSB"
    assert bad_dep.sum() <= max(1, int(1e-3 * npx)), f"{what}: {bad_dep.sum()} depths out of tolerance"
    assert (rgba[..., 3] == 255).all()
    return ids, id_r, dep


def _kinds(ids, env=None):
    m = ids >= lr.ID_ENV0
    if env is not None:
        m &= (ids - lr.ID_ENV0) // lr.IDS_PER_ENV == env
    return set(((ids[m] - lr.ID_ENV0) % lr.IDS_PER_ENV).tolist())


def test_render_returns_the_rgb_array_frame():
    env = _env(4)
    assert env.render_mode == "rgb_array" and "rgb_array" in env.metadata["render_modes"]
    env.reset()
    assert getattr(env, "_viewer_ws", None) is None            # the workspace is allocated on the first render
    img = env.render()
    assert env._viewer_ws is not None
    assert isinstance(img, np.ndarray) and img.shape == (720, 1280, 3) and img.dtype == np.uint8
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 10
    a = env.render_rgb()
    b = env.render_rgb()
    assert a.shape == (720, 1280, 4) and a.dtype == torch.uint8 and a.device.type == "cuda"
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)   # two rotating buffers, the same frame twice is bit-identical
    env.close()
    off = _env(4, render_mode=None)
    off.reset()
    assert off.render() is None
    off.close()
    vp = le.FrankaCubeLiftEnv(off.cfg, viewport=True)           # what the reference passes for --video
    assert vp.render_mode == "rgb_array"
    vp.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_kernel_matches_reference(case):
    ids, id_r, dep = _compare(case)
    name = case.name
    if name == "reset_closeup":
        assert len(_kinds(ids)) >= 10
    elif name == "posed5_world":
        assert {int(e) for e in np.unique((ids[ids >= lr.ID_ENV0] - lr.ID_ENV0) // lr.IDS_PER_ENV)} == {0, 1, 2, 3, 4}
    elif name == "posed5_env4":
        assert ((ids - lr.ID_ENV0) // lr.IDS_PER_ENV == 4).sum() > 500         # env 4 is what the camera is placed by
    elif name == "under_table":
        assert (ids == lr.ID_ENV0 + lr.K_TABLE).mean() > 0.5
    elif name.startswith("inside_segment"):
        k = int(name[-1])
        assert (ids == lr.ID_ENV0 + k).mean() > 0.5 and (ids == lr.ID_ENV0 + k + 1).sum() > 5
    elif name.startswith("ray_along"):
        h, w = ids.shape
        d = lr.vr.camera_rays(lr.f32(case.viewer.eye), lr.f32(case.viewer.lookat), w, h)[h // 2, w // 2]
        assert tuple(d) == ((1.0, 0.0, 0.0) if name.endswith("x") else (0.0, 1.0, 0.0))      # the centre ray is the axis itself
        assert ids[h // 2, w // 2] >= lr.ID_ENV0 and ids[h // 2, w // 2] == id_r[h // 2, w // 2]
    elif name == "no_targets":
        assert lr.K_GOAL not in _kinds(ids)
        env = _posed_env(dataclasses.replace(case, viewer=dataclasses.replace(case.viewer, draw_targets=True)))
        _, _, with_goals = _frame(env)
        env.close()
        goal = (with_goals >= lr.ID_ENV0) & ((with_goals - lr.ID_ENV0) % lr.IDS_PER_ENV == lr.K_GOAL)
        assert goal.sum() > 5 and (with_goals[~goal] == ids[~goal]).all()      # exactly the goals are gone
    elif name == "clips_cut":
        hit = np.isfinite(dep)
        assert hit.sum() > 50 and dep[hit].min() >= case.viewer.near_clip and dep[hit].max() <= case.viewer.far_clip
    elif name == "spacing_0.5":
        assert len({int(e) for e in np.unique((ids[ids >= lr.ID_ENV0] - lr.ID_ENV0) // lr.IDS_PER_ENV)}) == 5
    elif name == "cube_far_away":
        assert (ids == lr.ID_ENV0 + 2 * lr.IDS_PER_ENV + lr.K_CUBE).sum() > 20
    elif name == "nan_cube_and_joint":
        assert lr.K_CUBE not in _kinds(ids, 1) and lr.K_TABLE in _kinds(ids, 1)
        assert _kinds(ids, 3) <= {lr.K_TABLE, 1, 2, 3, 4, lr.K_CUBE, lr.K_GOAL} and {1, 3} <= _kinds(ids, 3)


def test_every_kind_is_hit_in_some_frame():
    seen = set()
    for name in ("gripper_closeup", "posed5_near", "inside_segment_1", "inside_segment_5"):
        env = _posed_env(next(c for c in CASES if c.name == name))
        seen |= _kinds(_frame(env)[2])
        env.close()
    assert seen == set(range(14)), seen


def test_rendering_does_not_perturb_the_simulation():
    runs = []
    for render in (True, False):
        env = _env(64, ViewerCfg(eye=(-6.0, -6.0, 3.5), resolution=(96, 64)), seed=11)
        env.reset()
        before = env.state.clone()
        if render:
            env.render()
            torch.cuda.synchronize()
            assert torch.equal(env.state.view(torch.int32), before.view(torch.int32))      # the state is bit-equal after a render
        g = torch.Generator(device=DEV).manual_seed(2)
        out = []
        for _ in range(20):
            o, r, te, tr, _ = env.step(torch.rand(64, 8, device=DEV, generator=g) * 2 - 1)
            out.append((o["policy"].clone(), r.clone(), te.clone(), tr.clone()))
            if render:
                env.render()
        out.append(env.get_state().clone())
        runs.append(out)
        env.close()
    for x, y in zip(runs[0][:-1], runs[1][:-1]):
        for u, w in zip(x, y):
            assert torch.equal(u, w)
    assert torch.equal(runs[0][-1].view(torch.int32), runs[1][-1].view(torch.int32))


def test_refusals_leave_the_outputs_untouched():
    n = 8
    env = _env(n, ViewerCfg(eye=(-6.0, -6.0, 3.5), resolution=(96, 64)))
    env.reset()
    env.render_rgb()
    lib = env._lib
    ws, nb = env._viewer_ws, env._viewer_ws_bytes
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    img = torch.full((64, 96), 0x01020304, dtype=torch.int32, device=DEV)
    dep = torch.full((64, 96), -7.0, device=DEV)
    ids = torch.full((64, 96), -5, dtype=torch.int32, device=DEV)
    native = lambda: le.lift_viewer_native(env.cfg.viewer, n, 2.5, 0.1034)        # noqa: E731

    def call(state=env.state, num=n, cfg=None, w=ws, wb=nb, rgba=img):
        cfg = native() if cfg is None else cfg
        return lib.rover_lift_viewer_render(_ptr(state) if isinstance(state, torch.Tensor) else state, num, C.byref(cfg),
                                            _ptr(w) if isinstance(w, torch.Tensor) else w, wb,
                                            _ptr(rgba) if isinstance(rgba, torch.Tensor) else rgba, _ptr(dep), _ptr(ids), st)

    def untouched():
        torch.cuda.synchronize()
        return bool((img == 0x01020304).all() and (dep == -7.0).all() and (ids == -5).all())

    assert call(state=None) == 1 and call(w=None) == 1 and call(rgba=None) == 1
    assert call(wb=nb - 1) == 1 and b"too small" in lib.rover_last_error()
    assert call(num=0) == 1 and call(num=-1) == 1
    host = np.zeros((_lib.LIFT_STATE_WORDS, n), np.float32)
    assert call(state=host.ctypes.data_as(C.c_void_p)) == 1                       # a state pointer that is not device memory
    for f in (lambda c: c.eye.__setitem__(0, float("nan")), lambda c: c.lookat.__setitem__(2, float("inf")),
              lambda c: [c.lookat.__setitem__(i, c.eye[i]) for i in range(3)],
              lambda c: [c.lookat.__setitem__(0, c.eye[0]), c.lookat.__setitem__(1, c.eye[1])],
              lambda c: setattr(c, "width", 0), lambda c: setattr(c, "height", 8193), lambda c: setattr(c, "focal_length", 0.0),
              lambda c: setattr(c, "horizontal_aperture", float("nan")), lambda c: setattr(c, "near_clip", -1.0),
              lambda c: setattr(c, "far_clip", 0.0), lambda c: setattr(c, "origin_type", 2),
              lambda c: setattr(c, "env_spacing", 0.0), lambda c: setattr(c, "ee_offset_z", float("nan")),
              lambda c: [setattr(c, "origin_type", 1), setattr(c, "env_index", n)],
              lambda c: [setattr(c, "origin_type", 1), setattr(c, "env_index", -1)]):
        c = native()
        f(c)
        assert call(cfg=c) == 1
        assert lib.rover_lift_viewer_workspace_bytes(n, C.byref(c)) == 0
    assert untouched()
    assert call() == 0                                                            # ... and the same buffers render
    torch.cuda.synchronize()
    assert (img.view(torch.uint8).view(64, 96, 4)[..., 3] == 255).all() and (ids >= 0).all() and (dep > 0).all()
    inf = native()
    inf.far_clip = float("inf")
    assert call(cfg=inf) == 0                                                     # far_clip may be +inf
    torch.cuda.synchronize()
    env.close()


def test_record_video_through_compat(tmp_path):
    import isaac_rover_orbit_amd.compat as compat
    gym = compat.gym_api()
    compat.register_default_tasks()
    cfg = le.LiftEnvCfg()
    cfg.scene.num_envs = 16
    cfg.sim.device = DEV
    cfg.viewer = ViewerCfg(eye=(-6.0, -6.0, 3.5), resolution=(160, 90))
    env = gym.make("FrankaCubeLift-v0", cfg=cfg, headless=True, viewport=True)
    assert env.unwrapped.render_mode == "rgb_array"
    folder = tmp_path / "videos"
    w = gym.wrappers.RecordVideo(env, video_folder=str(folder), step_trigger=lambda s: s == 0, video_length=10, disable_logger=True)
    w.reset()
    frames = [env.render()]
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(10):
        w.step(torch.rand(16, 8, device=DEV, generator=g) * 2 - 1)
        frames.append(env.render())
    files = sorted(os.listdir(folder))
    assert len(files) == 1 and files[0].endswith(".npz")
    rec = np.load(folder / files[0])["frames"]
    assert rec.shape == (10, 90, 160, 3) and rec.dtype == np.uint8
    assert np.array_equal(rec, np.stack(frames[:10]))
    assert len(np.unique(rec[0].reshape(-1, 3), axis=0)) > 10
    env.close()


def test_4096_envs_world_view():
    env = _env(4096)
    env.reset()
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(5):
        env.step(torch.rand(4096, 8, device=DEV, generator=g) * 2 - 1)
    env.render_frame()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rgba, dep, ids = env.render_frame(depth=True, object_id=True)
    torch.cuda.synchronize()
    assert _overflow(env) == 0                                 # the lattice walk finds every env
    print(f"4096 envs, 1280 x 720, world view: {1e3 * (time.perf_counter() - t0):.2f} ms (one frame, wall clock)")
    dep, ids = dep.cpu().numpy(), ids.cpu().numpy()
    assert ids.shape == (720, 1280) and ids.min() >= 0 and ids.max() < lr.ID_ENV0 + lr.IDS_PER_ENV * 4096
    assert ((ids - lr.ID_ENV0) % lr.IDS_PER_ENV)[ids >= lr.ID_ENV0].max() <= lr.K_GOAL
    assert not np.isnan(dep).any() and (dep > 0).all() and np.array_equal(np.isinf(dep), ids == lr.ID_SKY)
    assert len(np.unique((ids[ids >= lr.ID_ENV0] - lr.ID_ENV0) // lr.IDS_PER_ENV)) > 1       # more than one env is visible
    assert (rgba.cpu().numpy()[..., 3] == 255).all()
    env.close()


def test_one_camera_with_the_rover_viewer():
    """The two renderers agree on the camera, the sky and the packing: an all-sky view (the eye 5 m up, every ray at least 40 deg
    above the horizon, nothing either scene draws reaches z = 5) is the same bytes from both and is viewer_reference's sky formula,
    at sizes with one pixel, a whole tile and ragged tiles in either direction."""
    import test_gpu_viewer as rover
    import viewer_reference as vr
    eye, lookat = (0.0, 0.0, 5.0), (1.0, 0.0, 9.0)
    lift = _env(1)
    lift.reset()
    rov = rover._env(rover._terrain("flat", (64, 64)), 1)
    rov.reset()
    for w, h in ((1, 1), (8, 8), (9, 5), (17, 3)):
        lift.cfg.viewer = rov.cfg.viewer = ViewerCfg(eye=eye, lookat=lookat, resolution=(w, h))
        la, ld, li = _frame(lift)
        ra, rd, ri = (t.cpu().numpy() for t in rov.render_frame(depth=True, object_id=True))
        d = vr.camera_rays(eye, lookat, w, h)
        assert d[..., 2].min() > math.sin(math.radians(40.0))
        sky = np.asarray(vr.SKY_HORIZON) + (np.asarray(vr.SKY_ZENITH) - np.asarray(vr.SKY_HORIZON)) * np.maximum(d[..., 2:3], 0.0)
        assert la.shape == (h, w, 4) and la.tobytes() == ra.tobytes(), f"{w} x {h}"
        assert np.array_equal(la[..., :3], vr._byte(sky)) and (la[..., 3] == 255).all(), f"{w} x {h}"
        assert np.isposinf(ld).all() and np.isposinf(rd).all() and not li.any() and not ri.any(), f"{w} x {h}"
    lift.close()
    rov.close()
