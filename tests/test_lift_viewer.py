"""The lift viewer without a GPU: the float64 reference renderer (lift_viewer_reference.py) against the oracle's hand pose and the
rover reference's cylinder and sphere, the library's host entries (constants, env origins, config checks), the env's render
plumbing, and that every shared case (lift_viewer_cases.py) stays under the ambiguity cap the GPU test applies."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import lift_viewer_cases as lc
import lift_viewer_reference as lr
import viewer_reference as vr
from isaac_rover_orbit_amd import _lib
from isaac_rover_orbit_amd.cfg import ViewerCfg
from isaac_rover_orbit_amd.envs import lift_env as le

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS_T = 1e-4


@pytest.fixture(scope="module")
def lift_oracle():
    from oracle import lift_oracle
    lift_oracle.build()
    lift_oracle.lib()
    return lift_oracle


def _model_constants():
    lib = _lib.load()
    n = lib.rover_lift_model_constants(None, 0)
    out = np.zeros(n, np.float32)
    assert lib.rover_lift_model_constants(out.ctypes.data_as(C.c_void_p), n) == n
    return out


def _viewer_constants():
    lib = _lib.load()
    n = lib.rover_lift_viewer_constants(None, 0)
    out = np.zeros(n, np.float32)
    assert lib.rover_lift_viewer_constants(out.ctypes.data_as(C.c_void_p), n) == n
    return out


def test_reference_chain_end_is_the_oracles_hand_pose(lift_oracle):
    """tcp and hand R at 100 random joint vectors inside the limits.  The oracle is fp32: seven chained fp32 transforms of lengths
    under 1 m give about 1e-6; the bound is ten times that."""
    mc = _model_constants()
    lo, hi = mc[70:98:4], mc[71:98:4]                     # LF_Q_LO / LF_Q_HI of the table: (lo, hi, qd limit, effort) x 7 at 70
    assert np.array_equal(lo, lc.Q_LO) and np.array_equal(hi, lc.Q_HI)
    cfg = lift_oracle.default_config()
    rng = np.random.RandomState(0)
    worst_p = worst_r = 0.0
    for _ in range(100):
        q = np.zeros(9, np.float32)
        q[:7] = lo + (hi - lo) * rng.rand(7).astype(np.float32)
        tcp_o, R_o, _, _ = lift_oracle.hand_pose(cfg, q)
        tcp, R = lr.hand_pose(q[:7].astype(np.float64), float(np.float32(cfg.ee_offset_z)))
        worst_p = max(worst_p, np.abs(tcp - tcp_o).max())
        worst_r = max(worst_r, np.abs(R - R_o).max())
    print(f"chain end vs oracle: position {worst_p:.2e} m, rotation {worst_r:.2e}")
    assert worst_p <= 1e-5 and worst_r <= 1e-5


def test_viewer_constants_equal_the_model_constants():
    mc, v = _model_constants(), _viewer_constants()
    assert len(v) == 25
    for i in range(7):                                    # model table: (kind, a, d, mass) per DH row
        assert v[3 * i] == mc[4 * i] and v[3 * i + 1] == mc[4 * i + 1] and v[3 * i + 2] == mc[4 * i + 2], i
    s0 = 28 + 21 + 21 + 28 + 9                            # the scalars follow: K_GRAV, K_CUBE_HALF, K_CUBE_MASS, K_PAD_HALF_X, ...
    assert v[21] == mc[s0 + 16]                           # K_FLANGE_D
    assert v[22] == mc[s0 + 1] and v[23] == mc[s0 + 3] and v[24] == mc[s0 + 4]      # K_CUBE_HALF, K_PAD_HALF_X, K_PAD_HALF_Z
    # ... and the reference restates the same values
    f = np.float32
    assert [f(x) for x in v[0:21:3]] == [f(x) for x in lr.KIND]
    assert [f(x) for x in v[1:21:3]] == [f(x) for x in lr.DH_A] and [f(x) for x in v[2:21:3]] == [f(x) for x in lr.DH_D]
    assert list(v[21:]) == [f(lr.FLANGE_D), f(lr.CUBE_HALF), f(lr.PAD_HALF_X), f(lr.PAD_HALF_Z)]
    # a short buffer is filled as far as it goes
    few = np.full(4, -1.0, np.float32)
    assert _lib.load().rover_lift_viewer_constants(few.ctypes.data_as(C.c_void_p), 3) == 25
    assert list(few[:3]) == list(v[:3]) and few[3] == -1.0


def _defines(path):
    out = {}
    for name, val in re.findall(r"#define\s+(LR_\w+)\s+(.+?)(?:\s*//.*)?$", open(path).read(), flags=re.M):
        nums = [float(x.rstrip("f")) for x in re.findall(r"-?\d+\.?\d*(?:e-?\d+)?f?", val)]
        out[name] = nums if len(nums) > 1 else nums[0]
    return out


def test_reference_restates_the_rendering_constants():
    d = _defines(os.path.join(ROOT, "isaac_rover_orbit_amd", "csrc", "lift_render.hpp"))
    assert d["LR_TABLE_CENTER"] == list(lr.TABLE_CENTER) and d["LR_TABLE_HALF"] == list(lr.TABLE_HALF)
    assert d["LR_HAND_HALF"] == list(lr.HAND_HALF)
    assert (d["LR_ARM_RADIUS"], d["LR_HAND_CENTER_Z"], d["LR_FINGER_THICKNESS"], d["LR_FINGER_LENGTH"], d["LR_GOAL_RADIUS"],
            d["LR_GROUND_Z"]) == (lr.ARM_RADIUS, lr.HAND_CENTER_Z, lr.FINGER_THICKNESS, lr.FINGER_LENGTH, lr.GOAL_RADIUS, lr.GROUND_Z)
    for k, v in lr.ALBEDO.items():
        assert d["LR_ALBEDO_" + k.upper()] == list(v), k
    assert (d["LR_ID_SKY"], d["LR_ID_GROUND"], d["LR_ID_ENV0"], d["LR_IDS_PER_ENV"]) == (lr.ID_SKY, lr.ID_GROUND, lr.ID_ENV0, lr.IDS_PER_ENV)
    assert (d["LR_K_TABLE"], d["LR_K_ARM0"], d["LR_K_HAND"], d["LR_K_FINGER0"], d["LR_K_CUBE"], d["LR_K_GOAL"]) == \
        (lr.K_TABLE, lr.K_ARM0, lr.K_HAND, lr.K_FINGER0, lr.K_CUBE, lr.K_GOAL)
    # the table covers the cube's spawn range and the command range of the default cfg
    cfg = le.LiftEnvCfg()
    lo = np.array(lr.TABLE_CENTER) - lr.TABLE_HALF
    hi = np.array(lr.TABLE_CENTER) + lr.TABLE_HALF
    for i, (k, c) in enumerate((("x", "pos_x"), ("y", "pos_y"))):
        a, b = cfg.object_pose_range[k]
        assert lo[i] <= cfg.object_init_pos[i] + a - lr.CUBE_HALF * math.sqrt(3) and cfg.object_init_pos[i] + b + lr.CUBE_HALF * math.sqrt(3) <= hi[i]
        assert lo[i] <= cfg.command_ranges[c][0] and cfg.command_ranges[c][1] <= hi[i]
    assert hi[2] == 0.0


@pytest.mark.parametrize("n", [1, 2, 3, 5, 16, 17, 4096])
def test_env_origins_are_the_grid_cloners(n):
    spacing = 2.5
    out = np.full((n, 3), np.nan, np.float32)
    assert _lib.load().rover_lift_viewer_env_origins(n, spacing, out.ctypes.data_as(C.c_void_p)) == 0
    rows = math.ceil(n / int(math.sqrt(n)))
    cols = math.ceil(n / rows)
    for e in range(n):
        row, col = e // cols, e % cols
        x = (0.5 * (rows - 1) - row) * spacing
        y = (col - 0.5 * (cols - 1)) * spacing
        assert tuple(out[e]) == (np.float32(x), np.float32(y), np.float32(0.0)), e
    assert np.array_equal(lr.env_origins(n, spacing).astype(np.float32), out)


def test_env_origins_refuses_bad_arguments():
    lib = _lib.load()
    out = np.zeros(3, np.float32)
    assert lib.rover_lift_viewer_env_origins(0, 2.5, out.ctypes.data_as(C.c_void_p)) == 1
    assert lib.rover_lift_viewer_env_origins(1, 2.5, None) == 1
    assert lib.rover_lift_viewer_env_origins(1, float("nan"), out.ctypes.data_as(C.c_void_p)) == 1


def test_reference_capsule_is_a_cylinder_and_two_spheres():
    """On random rays from outside: the capsule's hit is the nearest of the rover reference's cylinder (radius WHEEL_RADIUS, half
    length WHEEL_HALF_WIDTH) and spheres about its two ends."""
    rng = np.random.RandomState(1)
    hits = 0
    for _ in range(20):
        c = rng.uniform(-1, 1, 3)
        a = rng.standard_normal(3)
        a /= np.linalg.norm(a)
        A, B = c - vr.WHEEL_HALF_WIDTH * a, c + vr.WHEEL_HALF_WIDTH * a
        M = 400
        o = c + rng.standard_normal((M, 3)) * 0.6
        far = np.linalg.norm(o - c, axis=1) > vr.WHEEL_HALF_WIDTH + vr.WHEEL_RADIUS + 0.02
        o = o[far]
        d = (c + rng.uniform(-0.25, 0.25, (len(o), 3))) - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        t, n = lr.capsule(o, d, A, B, vr.WHEEL_RADIUS, 0.0)
        tc, nc = vr._cylinder(o, d, c, a, 0.0)
        ta, na = vr._sphere(o, d, A, vr.WHEEL_RADIUS, 0.0)
        tb, nb = vr._sphere(o, d, B, vr.WHEEL_RADIUS, 0.0)
        # the cylinder's flat caps lie inside the end spheres, so the nearest of the three is the capsule's surface
        allt = np.stack([tc, ta, tb], 1)
        k = np.argmin(allt, 1)
        want = allt[np.arange(len(k)), k]
        assert np.array_equal(np.isfinite(t), np.isfinite(want))
        ok = np.isfinite(t)
        hits += ok.sum()
        assert np.abs(t[ok] - want[ok]).max() < 1e-12
        alln = np.stack([nc, na, nb], 1)[np.arange(len(k)), k]
        side_or_sphere = ok & ~((k == 0) & (np.abs((nc * a).sum(1)) > 0.5))      # not the cylinder's flat cap
        assert np.abs(n[side_or_sphere] - alln[side_or_sphere]).max() < 1e-9
    assert hits > 1000
    # a zero-length segment is a sphere
    o = rng.standard_normal((50, 3)) + 3
    d = -o / np.linalg.norm(o, axis=1, keepdims=True)
    t, n = lr.capsule(o, d, np.zeros(3), np.zeros(3), 0.2, 0.0)
    ts, ns = vr._sphere(o, d, np.zeros(3), 0.2, 0.0)
    assert np.array_equal(t, ts) and np.allclose(n, ns, atol=1e-12)


def test_cfg_metadata_and_viewport_mapping():
    cfg = le.LiftEnvCfg()
    assert isinstance(cfg.viewer, ViewerCfg) and tuple(cfg.viewer.eye) == (-6.0, -6.0, 3.5)         # manipulation_env_cfg.py:235
    assert cfg.viewer == ViewerCfg(eye=(-6.0, -6.0, 3.5))                                            # everything else default
    assert le.FrankaCubeLiftEnv.metadata == {"render_modes": [None, "rgb_array"]}
    kw = {"viewport": True, "other": 1}
    assert le.resolve_render_mode(None, kw) == "rgb_array" and kw == {"other": 1}
    assert le.resolve_render_mode(None, {"viewport": False}) is None
    assert le.resolve_render_mode(None, {}) is None
    assert le.resolve_render_mode("rgb_array", {}) == "rgb_array"
    for name in ("render", "render_rgb", "render_frame"):
        assert callable(getattr(le.FrankaCubeLiftEnv, name))


def test_native_config_mirrors_the_cfg_and_validates():
    lib = _lib.load()
    d = _lib.LiftViewerConfig()
    assert lib.rover_lift_viewer_default_config(C.byref(d)) == 0
    assert lib.rover_lift_viewer_config_bytes() == C.sizeof(_lib.LiftViewerConfig)
    cfg = le.LiftEnvCfg()
    c = le.lift_viewer_native(cfg.viewer, 16, cfg.scene.env_spacing, cfg.ee_offset_z)
    for name, _ in _lib.LiftViewerConfig._fields_:
        a, b = getattr(d, name), getattr(c, name)
        assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), name
    assert (d.env_spacing, d.ee_offset_z, d.draw_targets) == (2.5, np.float32(0.1034), 1)
    assert lib.rover_lift_viewer_workspace_bytes(16, C.byref(c)) > 16 * 64 * 4
    v = ViewerCfg(eye=(1.0, 2.0, 3.0), lookat=(0.5, 0.0, 0.2), resolution=(96, 64), origin_type="env", env_index=3, draw_targets=False,
                  near_clip=0.5, far_clip=float("inf"))
    c = le.lift_viewer_native(v, 4, 0.5, 0.2)
    assert (c.origin_type, c.env_index, c.width, c.height, c.draw_targets, c.env_spacing, math.isinf(c.far_clip)) == \
        (_lib.VIEWER_ORIGIN_ENV, 3, 96, 64, 0, 0.5, True)
    # ViewerCfg.validate is the gate
    for bad in (ViewerCfg(eye=(0, 0, 1), lookat=(0, 0, 0)), ViewerCfg(resolution=(0, 64)), ViewerCfg(near_clip=2.0, far_clip=1.0),
                ViewerCfg(origin_type="env", env_index=4), ViewerCfg(focal_length=0.0), ViewerCfg(eye=(float("nan"), 0, 0))):
        with pytest.raises(ValueError):
            le.lift_viewer_native(bad, 4, 2.5, 0.1034)
    with pytest.raises(ValueError):
        le.lift_viewer_native(ViewerCfg(), 4, 0.0, 0.1034)
    # workspace_bytes: 0 for an invalid cfg or num_envs <= 0
    good = le.lift_viewer_native(ViewerCfg(), 4, 2.5, 0.1034)
    assert lib.rover_lift_viewer_workspace_bytes(0, C.byref(good)) == 0 and lib.rover_lift_viewer_workspace_bytes(-3, C.byref(good)) == 0
    assert lib.rover_lift_viewer_workspace_bytes(4, None) == 0
    for f in (lambda c: setattr(c, "env_spacing", 0.0), lambda c: setattr(c, "env_spacing", float("inf")),
              lambda c: setattr(c, "ee_offset_z", float("nan")), lambda c: setattr(c, "width", 8193),
              lambda c: [setattr(c, "origin_type", 1), setattr(c, "env_index", 4)]):
        c = le.lift_viewer_native(ViewerCfg(), 4, 2.5, 0.1034)
        f(c)
        assert lib.rover_lift_viewer_workspace_bytes(4, C.byref(c)) == 0


@pytest.mark.parametrize("case", lc.cases(), ids=lambda c: c.name)
def test_reference_alone_stays_under_the_ambiguity_cap(case, lift_oracle):
    S = case.state
    if S is None:
        S = lift_oracle.new_state(case.n)
        lift_oracle.reset(lift_oracle.default_config(), S)
    _, dep, ids, gap, graze = lr.render(case.viewer, S, case.env_spacing, lc.EE_OFFSET_Z)
    amb = (gap < EPS_T * (1 + np.where(np.isfinite(dep), dep, 0))) | graze
    print(f"{case.name}: {int(amb.sum())} of {ids.size} pixels ambiguous")
    assert amb.sum() < 0.02 * ids.size
    assert (ids >= lr.ID_ENV0).sum() > 20                   # the scene is in the picture


def test_reference_cases_hit_every_kind_and_leave_nan_parts_out(lift_oracle):
    cs = {c.name: c for c in lc.cases()}
    seen = set()
    for name in ("gripper_closeup", "posed5_near", "inside_segment_1", "inside_segment_5"):
        c = cs[name]
        ids = lr.render(c.viewer, c.state, c.env_spacing, lc.EE_OFFSET_Z)[2]
        seen |= set(((ids[ids >= lr.ID_ENV0] - lr.ID_ENV0) % lr.IDS_PER_ENV).tolist())
    assert seen == set(range(14))
    c = cs["nan_cube_and_joint"]
    kinds = lambda e: {p[0] for p in lr.primitives(c.state[e], np.zeros(3), lc.EE_OFFSET_Z)}     # noqa: E731
    assert kinds(0) == set(range(14))
    assert kinds(1) == set(range(14)) - {lr.K_CUBE}
    # joint 3 (0-based) is NaN: frame origins p1 .. p4 do not depend on it, everything after does
    assert kinds(3) == {lr.K_TABLE, 1, 2, 3, 4, lr.K_CUBE, lr.K_GOAL}
