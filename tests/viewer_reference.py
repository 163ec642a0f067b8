"""Float64 reference of the rgb_array viewer: shares no code with viewer_kernels.hip.

Terrain hits come from ``camera_reference.cast_brute`` (every ray against the mesh's triangle list); the hit triangle is found
from the hit point.  Rovers and targets are tested analytically (ray-box, ray-cylinder, ray-sphere) over every env.  Wheel poses
come from ``tests/golden/rover_model.json`` and the state words, not from the kernel's constants.  The rendering constants are
restated here; ``test_viewer.py`` checks them against ``csrc/rover_render.hpp``.
"""
from __future__ import annotations

import json
import os

import numpy as np

from camera_reference import cast_brute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = json.load(open(os.path.join(ROOT, "tests", "golden", "rover_model.json")))

# state words (include/rover_hip.h)
POS, QUAT, BOGIE_Q, STEER_Q, TARGET_W = 0, 3, 13, 16, 39

# ---- rendering constants (csrc/rover_render.hpp)
CHASSIS_CENTER = (0.0, 0.0, 0.06)
CHASSIS_HALF = (0.36, 0.22, 0.08)
WHEEL_HALF_WIDTH = 0.05
TARGET_RADIUS = 0.12
TARGET_Z_OFFSET = 0.30
FOCAL_LENGTH = 18.147562
HORIZONTAL_APERTURE = 20.955
NEAR_CLIP = 0.01
FAR_CLIP = 1000000.0
LIGHT_POS = (0.0, -180.0, 80.0)
K_AMBIENT = 0.35
K_DIFFUSE = 0.65
ALBEDO = {"ground": (0.62, 0.52, 0.40), "rock": (0.42, 0.40, 0.40), "chassis": (0.85, 0.85, 0.88), "wheel": (0.14, 0.14, 0.15),
          "target": (0.95, 0.22, 0.16)}
ROCK_EPS = 1.0e-3
SKY_HORIZON = (0.80, 0.85, 0.92)
SKY_ZENITH = (0.36, 0.56, 0.86)
ID_SKY, ID_GROUND, ID_ROCK, ID_ENV0, IDS_PER_ENV = 0, 1, 2, 3, 8

WHEELS = ("FL", "FR", "CL", "CR", "RL", "RR")          # object id order 1..6
STEER = {"FL": 0, "FR": 1, "RL": 2, "RR": 3}            # steer joint order of the state words
BOGIES = ("FL_Boogie", "FR_Boogie", "R_Boogie")
WHEEL_RADIUS = float(MODEL["wheel_contact_radius"])


def quat_to_mat(q):
    q = np.asarray(q, np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def axis_angle(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def rover_parts(state_row):
    """World pose of one env's parts: (pos, R, wheel centres (6, 3), wheel axles (6, 3)) from the state words."""
    s = np.asarray(state_row, np.float64)
    pos, R = s[POS:POS + 3], quat_to_mat(s[QUAT:QUAT + 4])
    cen, axl = [], []
    for k, w in enumerate(WHEELS):
        b = MODEL["wheel_bogie"][w]
        j = BOGIES.index(b)
        Rb = axis_angle(MODEL["bogies"][b]["axis"], s[BOGIE_Q + j])
        P = np.array(MODEL["bogies"][b]["pivot"])
        c = P + Rb @ (np.array(MODEL["wheel_centres"][w]) - P)
        a = np.array(MODEL["drive_axis"][w], np.float64)
        a = a / np.linalg.norm(a)
        if w in STEER:
            a = axis_angle(MODEL["steer_axis"][w], s[STEER_Q + STEER[w]]) @ a
        cen.append(pos + R @ c)
        axl.append(R @ (Rb @ a))
    return pos, R, np.array(cen), np.array(axl)


def camera_rays(eye, lookat, width, height, focal_length=FOCAL_LENGTH, horizontal_aperture=HORIZONTAL_APERTURE):
    """Unit ray directions (height, width, 3) through the pixel centres; row 0 at the top."""
    f = np.asarray(lookat, np.float64) - np.asarray(eye, np.float64)
    f /= np.linalg.norm(f)
    r = np.array([f[1], -f[0], 0.0])
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    fpx = width * focal_length / horizontal_aperture
    x = (np.arange(width) + 0.5 - 0.5 * width) / fpx
    y = -(np.arange(height) + 0.5 - 0.5 * height) / fpx
    d = f[None, None, :] + x[None, :, None] * r[None, None, :] + y[:, None, None] * u[None, None, :]
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _pick(t0, t1, near):
    """The ray's surface hit of an interval [t0, t1]: t0 if it is past the near clip, else t1 (the ray starts inside)."""
    front = t0 >= near
    t = np.where(front, t0, t1)
    return np.where((t0 <= t1) & (t >= near), t, np.inf), front


def _box(o, d, pos, R, near, grow=0.0):
    """o, d (M, 3); pos (M, 3); R (M, 3, 3): t (M,), normal (M, 3) facing the ray."""
    c, h = np.array(CHASSIS_CENTER), np.array(CHASSIS_HALF) + grow
    ol = np.einsum("mji,mj->mi", R, o - pos) - c
    dl = np.einsum("mji,mj->mi", R, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / dl
        ta, tb = (-h - ol) * inv, (h - ol) * inv
    par = dl == 0
    inside = np.abs(ol) <= h
    lo = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(ta, tb))
    hi = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(ta, tb))
    te, tx = lo.max(1), hi.min(1)
    ae, ax = lo.argmax(1), hi.argmin(1)
    t, front = _pick(te, tx, near)
    a = np.where(front, ae, ax)
    m = np.arange(len(a))
    s = np.where(dl[m, a] > 0, -1.0, 1.0)
    n = R[m, :, a] * s[:, None]
    return t, n


def _cylinder(o, d, c, a, near, grow=0.0):
    r, hw = WHEEL_RADIUS + grow, WHEEL_HALF_WIDTH + grow
    oc = o - c
    dpar, opar = (d * a).sum(1), (oc * a).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s0, s1 = (-hw - opar) / dpar, (hw - opar) / dpar
    par = dpar == 0
    ins = np.abs(opar) <= hw
    sa = np.where(par, np.where(ins, -np.inf, np.inf), np.minimum(s0, s1))
    sb = np.where(par, np.where(ins, np.inf, -np.inf), np.maximum(s0, s1))
    dp, op = d - dpar[:, None] * a, oc - opar[:, None] * a
    A, B, C = (dp * dp).sum(1), (op * dp).sum(1), (op * op).sum(1) - r * r
    disc = B * B - A * C
    with np.errstate(divide="ignore", invalid="ignore"):
        sq = np.sqrt(np.maximum(disc, 0))
        q0, q1 = (-B - sq) / A, (-B + sq) / A
    zero = A == 0
    q0 = np.where(zero, np.where(C <= 0, -np.inf, np.inf), np.where(disc >= 0, q0, np.inf))
    q1 = np.where(zero, np.where(C <= 0, np.inf, -np.inf), np.where(disc >= 0, q1, -np.inf))
    te, tx = np.maximum(sa, q0), np.minimum(sb, q1)
    t, front = _pick(te, tx, near)
    cap = np.where(front, sa > q0, sb < q1)
    x = oc + np.where(np.isfinite(t), t, 0)[:, None] * d
    side = x - (x * a).sum(1)[:, None] * a
    side /= np.maximum(np.linalg.norm(side, axis=1, keepdims=True), 1e-300)
    n = np.where(cap[:, None], a, side)
    n = n * np.where((n * d).sum(1) > 0, -1.0, 1.0)[:, None]
    return t, n


def _sphere(o, d, c, r, near):
    oc = o - c
    b, cc = (oc * d).sum(1), (oc * oc).sum(1) - r * r
    disc = b * b - cc
    sq = np.sqrt(np.maximum(disc, 0))
    t0, t1 = np.where(disc >= 0, -b - sq, np.inf), np.where(disc >= 0, -b + sq, -np.inf)
    t, _ = _pick(t0, t1, near)
    x = oc + np.where(np.isfinite(t), t, 0)[:, None] * d
    n = x / r
    n = n * np.where((n * d).sum(1) > 0, -1.0, 1.0)[:, None]
    return t, n


def object_hits(o, d, state, draw_targets=True, near=NEAR_CLIP, grow=0.0):
    """Every env's parts against rays o, d (M, 3): t (M, 8 N), normals (M, 8 N, 3), ids (8 N,).  `grow` widens every part (the
    ambiguity test renders with +-grow)."""
    M = o.shape[0]
    # envs some ray passes within 1.5 m of (rover root or target): the others cannot be hit (their parts lie within 0.7 m)
    keep = []
    for e in range(state.shape[0]):
        for c in (state[e, POS:POS + 3], state[e, TARGET_W:TARGET_W + 3] + [0, 0, TARGET_Z_OFFSET]):
            w = c - o
            along = np.maximum((w * d).sum(1), 0.0)
            if (np.linalg.norm(w - along[:, None] * d, axis=1) < 1.5).any():
                keep.append(e)
                break
    T = np.full((M, IDS_PER_ENV * len(keep)), np.inf)
    Nn = np.zeros((M, IDS_PER_ENV * len(keep), 3))
    ids = (ID_ENV0 + IDS_PER_ENV * np.asarray(keep, np.int64)[:, None] + np.arange(IDS_PER_ENV)[None, :]).reshape(-1)
    for i, e in enumerate(keep):
        pos, R, cen, axl = rover_parts(state[e])
        k0 = IDS_PER_ENV * i
        T[:, k0], Nn[:, k0] = _box(o, d, np.broadcast_to(pos, o.shape), np.broadcast_to(R, (M, 3, 3)), near, grow)
        for k in range(6):
            T[:, k0 + 1 + k], Nn[:, k0 + 1 + k] = _cylinder(o, d, cen[k], axl[k], near, grow)
        if draw_targets:
            c = np.asarray(state[e, TARGET_W:TARGET_W + 3], np.float64) + [0, 0, TARGET_Z_OFFSET]
            T[:, k0 + 7], Nn[:, k0 + 7] = _sphere(o, d, c, TARGET_RADIUS + grow, near)
    return T, Nn, ids


def _byte(x):
    return np.rint(255.0 * np.clip(x, 0.0, 1.0)).astype(np.uint8)


def render_rays(o, d, height, obstacle, res, min_x, min_y, state, draw_targets=True, near=NEAR_CLIP, far=FAR_CLIP, eps=1e-4):
    """rgb (M, 3) uint8, depth (M,), id (M,), gap (M,) for rays o, d (M, 3): `gap` is the distance between the nearest hit and the
    nearest hit of ANOTHER object (inf if none), and `graze` marks rays whose id changes when every rover part and target grows
    or shrinks by `eps` metres (silhouette pixels) -- the two conditions under which an fp32 renderer may pick another object."""
    h = np.asarray(height, np.float64)
    ob = None if obstacle is None else np.asarray(obstacle, np.float64)
    t_ter = cast_brute(h, res, min_x, min_y, o, d, near, far)
    T, Nn, ids = object_hits(o, d, state, draw_targets, near)
    T = np.where(T <= far, T, np.inf)
    allT = np.concatenate([t_ter[:, None], T], 1)
    allid = np.concatenate([[ID_GROUND], ids])
    # nearest: smallest t, ties to the lower id (allid is increasing, argmin takes the first)
    k = np.argmin(allT, 1)
    m = np.arange(len(k))
    depth = allT[m, k]
    hit = np.isfinite(depth)
    oid = np.where(hit, allid[k], ID_SKY)
    srt = np.sort(np.concatenate([allT, np.full((len(k), 1), np.inf)], 1), 1)
    with np.errstate(invalid="ignore"):
        gap = np.where(hit, srt[:, 1] - srt[:, 0], np.inf)
    graze = np.zeros(len(k), bool)
    for g in (eps, -eps):
        Tg, _, _ = object_hits(o, d, state, draw_targets, near, grow=g)
        Tg = np.where(Tg <= far, Tg, np.inf)
        aT = np.concatenate([t_ter[:, None], Tg], 1)
        kg = np.argmin(aT, 1)
        og = np.where(np.isfinite(aT[m, kg]), allid[kg], ID_SKY)
        graze |= og != oid
    # shading
    n = np.zeros((len(k), 3))
    X = o + np.where(hit, depth, 0)[:, None] * d
    ter = hit & (k == 0)
    rock = np.zeros(len(k), bool)
    if ter.any():
        H, W = h.shape
        gx, gy = (X[ter, 0] - min_x) / res, (X[ter, 1] - min_y) / res
        ix, iy = np.clip(np.floor(gx).astype(int), 0, W - 2), np.clip(np.floor(gy).astype(int), 0, H - 2)
        fx, fy = gx - ix, gy - iy
        lower = fx >= fy
        h00, h01, h10, h11 = h[iy, ix], h[iy, ix + 1], h[iy + 1, ix], h[iy + 1, ix + 1]
        a = np.where(lower, h01 - h00, h11 - h10)
        b = np.where(lower, h11 - h01, h10 - h00)
        nt = np.stack([-a / res, -b / res, np.ones_like(a)], 1)
        nt /= np.linalg.norm(nt, axis=1, keepdims=True)
        n[ter] = nt
        if ob is not None:
            om = np.maximum(np.maximum(ob[iy, ix], ob[iy + 1, ix + 1]), np.where(lower, ob[iy, ix + 1], ob[iy + 1, ix]))
            r_ = np.zeros(len(k), bool)
            r_[ter] = om > ROCK_EPS
            rock = r_
    objs = hit & (k > 0)
    n[objs] = Nn[m[objs], k[objs] - 1]
    n *= np.where((n * d).sum(1) > 0, -1.0, 1.0)[:, None]
    oid = np.where(rock, ID_ROCK, oid)
    kind = np.where(oid >= ID_ENV0, (oid - ID_ENV0) % IDS_PER_ENV, -1)
    alb = np.zeros((len(k), 3))
    alb[oid == ID_GROUND] = ALBEDO["ground"]
    alb[oid == ID_ROCK] = ALBEDO["rock"]
    alb[kind == 0] = ALBEDO["chassis"]
    alb[(kind >= 1) & (kind <= 6)] = ALBEDO["wheel"]
    alb[kind == 7] = ALBEDO["target"]
    L = np.asarray(LIGHT_POS) - X
    L /= np.linalg.norm(L, axis=1, keepdims=True)
    shade = K_AMBIENT + K_DIFFUSE * np.maximum((n * L).sum(1), 0.0)
    rgb = alb * shade[:, None]
    sky = np.asarray(SKY_HORIZON) + (np.asarray(SKY_ZENITH) - np.asarray(SKY_HORIZON)) * np.maximum(d[:, 2:3], 0.0)
    rgb = np.where(hit[:, None], rgb, sky)
    return _byte(rgb), np.where(hit, depth, np.inf), oid, gap, graze


def render(viewer, height, obstacle, res, min_x, min_y, state, pixels=None):
    """The frame of `viewer` (a ViewerCfg) for `state` (N, 72): rgb (H, W, 3) uint8, depth (H, W), id (H, W), gap (H, W), graze
    (H, W) -- or, with `pixels` = (rows, cols) index arrays, those pixels only (1-D arrays)."""
    W, H = viewer.resolution
    state = np.asarray(state, np.float64)
    # the basis from the fp32 values of eye / lookat as the C struct holds them (origin "env" shifts both: the basis is the same)
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)    # noqa: E731
    d = camera_rays(f32(viewer.eye), f32(viewer.lookat), W, H, viewer.focal_length, viewer.horizontal_aperture)
    eye = f32(viewer.eye)
    if viewer.origin_type == "env":
        eye = eye + state[viewer.env_index, POS:POS + 3]
    if pixels is not None:
        d = d[pixels[0], pixels[1]]
    else:
        d = d.reshape(-1, 3)
    o = np.broadcast_to(eye, d.shape).copy()
    out = render_rays(o, d, height, obstacle, res, min_x, min_y, state, viewer.draw_targets, viewer.near_clip, viewer.far_clip)
    if pixels is not None:
        return out
    rgb, dep, oid, gap, graze = out
    return rgb.reshape(H, W, 3), dep.reshape(H, W), oid.reshape(H, W), gap.reshape(H, W), graze.reshape(H, W)
