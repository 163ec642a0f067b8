"""The posed scenes the CPU test (test_lift_viewer.py: the reference alone stays under the ambiguity cap) and the GPU test
(test_gpu_lift_viewer.py: kernel against reference) of the lift viewer share.  Frames are 96 x 64 unless a case says otherwise (the
axis-ray cases need an odd size for a centre pixel, the 29-env lattice case is 64 x 48 to keep the brute-force reference quick).

A case: name, n (envs), state (an (n, 64) float32 array, or None = "after reset()": the CPU test takes the oracle's reset, the GPU
test the env's), the ViewerCfg, env_spacing."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import lift_viewer_reference as lr
from isaac_rover_orbit_amd.cfg import ViewerCfg

Q_DEFAULT = np.array([0.0, -0.569, 0.0, -2.810, 0.0, 3.037, 0.741, 0.04, 0.04], np.float32)       # FRANKA_PANDA_CFG init_state
Q_LO = np.array([-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973], np.float32)     # LF_Q_LO / LF_Q_HI
Q_HI = np.array([2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973], np.float32)
EE_OFFSET_Z = 0.1034
RES = (96, 64)


@dataclass
class Case:
    name: str
    n: int
    state: np.ndarray | None
    viewer: ViewerCfg
    env_spacing: float = 2.5


def quat(yaw=0.0, pitch=0.0, roll=0.0):
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    return [cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy]


def rows(n, specs=()):
    """(n, 64) float32: every env in the default pose with the cube at rest at (0.5, 0, 0.02) and the goal at (0.5, 0.5, 0);
    specs[e] = dict(q=, fingers=, cube=, quat=, goal=) overrides env e."""
    S = np.zeros((n, lr.STATE_WORDS), np.float32)
    S[:, lr.Q:lr.Q + 9] = Q_DEFAULT
    S[:, lr.OBJ_POS:lr.OBJ_POS + 3] = (0.5, 0.0, 0.02)
    S[:, lr.OBJ_QUAT] = 1.0
    S[:, lr.CMD:lr.CMD + 3] = (0.5, 0.5, 0.0)
    S[:, lr.CMD + 3] = 1.0
    for e, sp in enumerate(specs):
        if "q" in sp:
            S[e, lr.Q:lr.Q + 7] = sp["q"]
        if "fingers" in sp:
            S[e, lr.Q + 7:lr.Q + 9] = sp["fingers"]
        if "cube" in sp:
            S[e, lr.OBJ_POS:lr.OBJ_POS + 3] = sp["cube"]
        if "quat" in sp:
            S[e, lr.OBJ_QUAT:lr.OBJ_QUAT + 4] = sp["quat"]
        if "goal" in sp:
            S[e, lr.CMD:lr.CMD + 3] = sp["goal"]
    return S


_rng = np.random.RandomState(7)
POSED5 = [  # joints at both limits, fingers open and closed, cube rotated and lifted, goal in the air
    dict(q=Q_LO, fingers=(0.04, 0.04), cube=(0.5, 0.1, 0.30), quat=quat(0.7, 0.4, -0.3), goal=(0.5, 0.4, 0.40)),
    dict(q=Q_HI, fingers=(0.0, 0.0), cube=(0.45, -0.2, 0.02), quat=quat(1.1), goal=(0.4, -0.3, 0.25)),
    dict(fingers=(0.025, 0.015), cube=(0.55, 0.15, 0.12), quat=quat(-0.5, 0.9, 0.2), goal=(0.6, 0.5, 0.30)),
    dict(q=Q_LO + (Q_HI - Q_LO) * _rng.rand(7).astype(np.float32), fingers=(0.01, 0.03), goal=(0.3, 0.3, 0.10)),
    dict(q=Q_LO + (Q_HI - Q_LO) * _rng.rand(7).astype(np.float32), fingers=(0.04, 0.0), cube=(0.6, -0.1, 0.2), quat=quat(0.2, -1.0, 2.0)),
]


def _default_points():
    pts, X, Y, Z = lr.chain(Q_DEFAULT[:7].astype(np.float64))
    return pts, pts[7] + Z * (lr.FLANGE_D + EE_OFFSET_Z)


def cases():
    P, tcp = _default_points()
    V = lambda eye, at, **kw: ViewerCfg(eye=tuple(float(x) for x in eye), lookat=tuple(float(x) for x in at),     # noqa: E731
                                        resolution=kw.pop("resolution", RES), **kw)
    nan_rows = rows(5, POSED5)
    nan_rows[1, lr.OBJ_POS + 1] = np.nan                # env 1's cube has a NaN position
    nan_rows[3, lr.Q + 3] = np.nan                      # env 3's arm has a NaN joint
    far_rows = rows(5, POSED5)
    far_rows[2, lr.OBJ_POS:lr.OBJ_POS + 3] = (0.5, 7.5, 0.3)    # env 2 sits at (0, -1.25): its cube is 3 spacings away along +y
    seg5_mid = 0.5 * (P[4] + P[5])
    return [
        Case("reset_closeup", 1, None, V((1.6, -1.2, 0.9), (0.4, 0.0, 0.3))),
        Case("gripper_closeup", 1, rows(1, [dict(fingers=(0.03, 0.02))]), V(tcp + (0.22, -0.26, 0.08), tcp)),
        Case("posed5_world", 5, rows(5, POSED5), V((-5.0, -4.0, 3.0), (0.0, 0.0, 0.3))),
        Case("posed5_near", 5, rows(5, POSED5), V((1.9, -3.4, 1.3), (0.5, -1.25, 0.4))),
        Case("posed5_env4", 5, rows(5, POSED5), V((1.8, -1.5, 1.0), (0.4, 0.0, 0.3), origin_type="env", env_index=4)),
        Case("under_table", 1, rows(1), V((0.6, 0.4, -0.7), (0.3, 0.0, 0.0))),
        Case("inside_segment_1", 1, rows(1), V((0.03, 0.0, 0.12), (0.03 + 0.438, 0.0, 0.12 + 0.899))),
        Case("inside_segment_5", 1, rows(1), V(seg5_mid, seg5_mid + (0.5, 0.45, -0.05))),
        Case("ray_along_x", 2, rows(2), V((-3.5, 0.0, 0.4), (0.0, 0.0, 0.4), resolution=(95, 63))),
        Case("ray_along_y", 2, rows(2), V((1.75, -2.0, 0.02), (1.75, 0.0, 0.02), resolution=(95, 63))),
        Case("no_targets", 5, rows(5, POSED5), V((1.5, -1.9, 0.9), (0.55, -0.9, 0.3), draw_targets=False)),
        Case("clips_cut", 5, rows(5, POSED5), V((1.9, -3.4, 1.3), (0.5, -1.25, 0.4), near_clip=2.45, far_clip=3.1)),
        Case("spacing_0.5", 5, rows(5, POSED5), V((-2.6, 0.15, 0.04), (0.3, 0.0, 0.4)), env_spacing=0.5),
        Case("cube_far_away", 5, far_rows, V((0.6, 6.95, 0.36), (0.5, 6.25, 0.3))),
        Case("lattice29_grazing", 29, rows(29, [POSED5[e % 5] for e in range(29)]), V((-8.5, -7.0, 1.1), (0.0, 0.3, 0.3), resolution=(64, 48))),
        Case("nan_cube_and_joint", 5, nan_rows, V((-2.2, 3.6, 1.8), (1.25, 1.25, 0.3))),
    ]
