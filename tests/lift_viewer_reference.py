"""Float64 reference of the FrankaCubeLift-v0 rgb_array viewer: shares no code with
lift_viewer_kernels.hip and no traversal -- every ray is tested against every primitive of every env.

The camera rays, the ray-sphere test and the byte rounding are viewer_reference.py's (the rover viewer's float64 reference).  The
model data (modified-DH rows, flange, cube and pad sizes) and the rendering constants are restated here; test_lift_viewer.py
checks the former against ``rover_lift_model_constants`` and the latter against ``csrc/lift_render.hpp``.
"""
from __future__ import annotations

import numpy as np

import viewer_reference as vr

# state words (include/rover_lift.h)
Q, OBJ_POS, OBJ_QUAT, CMD, STATE_WORDS = 0, 18, 21, 31, 64

# ---- model data (csrc/lift_kernels.hip; the viewer's copies are in csrc/lift_render.hpp)
KIND = (0, -1, 1, 1, -1, 1, 1)
DH_A = (0.0, 0.0, 0.0, 0.0825, -0.0825, 0.0, 0.088)
DH_D = (0.333, 0.0, 0.316, 0.0, 0.384, 0.0, 0.0)
FLANGE_D, CUBE_HALF, PAD_HALF_X, PAD_HALF_Z = 0.107, 0.02, 0.010, 0.009

# ---- rendering constants (csrc/lift_render.hpp)
ARM_RADIUS = 0.055
TABLE_CENTER = (0.35, 0.0, -0.03)
TABLE_HALF = (0.65, 0.85, 0.03)
HAND_CENTER_Z = 0.033
HAND_HALF = (0.0315, 0.102, 0.033)
FINGER_THICKNESS = 0.012
FINGER_LENGTH = 0.030
GOAL_RADIUS = 0.03
GROUND_Z = -1.05
ALBEDO = {"ground": (0.55, 0.55, 0.56), "table": (0.60, 0.45, 0.30), "arm": (0.90, 0.90, 0.92), "hand": (0.80, 0.80, 0.84),
          "finger": (0.20, 0.20, 0.22), "cube": (0.20, 0.45, 0.85), "goal": (0.95, 0.22, 0.16)}
ID_SKY, ID_GROUND, ID_ENV0, IDS_PER_ENV = 0, 1, 2, 16
K_TABLE, K_ARM0, K_HAND, K_FINGER0, K_CUBE, K_GOAL = 0, 1, 9, 10, 12, 13
KIND_ALBEDO = ["table"] + ["arm"] * 8 + ["hand", "finger", "finger", "cube", "goal"]


def f32(x):
    """The value as a float32 C field holds it, in float64."""
    return np.asarray(x, np.float32).astype(np.float64)


def env_origins(n, spacing):
    """Isaac's grid cloner (ASSUMED, section 29): (n, 3)."""
    rows = int(np.ceil(n / int(np.sqrt(n))))
    cols = int(np.ceil(n / rows))
    e = np.arange(n)
    row, col = e // cols, e % cols
    return np.stack([(0.5 * (rows - 1) - row) * spacing, (col - 0.5 * (cols - 1)) * spacing, np.zeros(n)], 1)


def chain(q7):
    """Modified-DH chain (Craig): frame origins base, p1 .. p7 (8, 3) and the last frame's axes X, Y, Z, in the base frame."""
    T = np.eye(4)
    pts = [np.zeros(3)]
    with np.errstate(invalid="ignore"):
        for i in range(7):
            al = KIND[i] * np.pi / 2
            ca, sa = round(np.cos(al)), round(np.sin(al))
            ct, st = np.cos(q7[i]), np.sin(q7[i])
            # p_i does not depend on q_i: translate in the parent frame first (a along x, then d along the rotated z) ...
            off = np.array([DH_A[i], -sa * DH_D[i], ca * DH_D[i]])
            pts.append(T[:3, 3] + T[:3, :3] @ off)
            # ... then Rx(alpha) Rz(theta)
            A = np.array([[ct, -st, 0, DH_A[i]],
                          [st * ca, ct * ca, -sa, -sa * DH_D[i]],
                          [st * sa, ct * sa, ca, ca * DH_D[i]],
                          [0, 0, 0, 1.0]])
            T = T @ A
    return np.array(pts), T[:3, 0], T[:3, 1], T[:3, 2]


def hand_pose(q7, ee_offset_z):
    """tcp (3,) and hand R (3, 3; columns x_hand, y_hand, z_hand) of the contract -- what the step's hand_kinematics computes."""
    pts, X, Y, Z = chain(np.asarray(q7, np.float64))
    R = np.stack([(X - Y) / np.sqrt(2), (X + Y) / np.sqrt(2), Z], 1)
    return pts[7] + Z * (FLANGE_D + ee_offset_z), R


def quat_to_matrix(q):
    """The step's quat_to_matrix: the quaternion as stored, no normalisation."""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def primitives(row, origin, ee_offset_z, draw_targets=True):
    """One env's drawn primitives as (k, kind, params): ("box", centre, G rows, half), ("capsule", A, B, radius),
    ("sphere", centre, radius).  A primitive with a non-finite parameter is left out."""
    s = np.asarray(row, np.float64)
    origin = np.asarray(origin, np.float64)
    fin = lambda *a: all(np.isfinite(np.asarray(x)).all() for x in a)        # noqa: E731
    out = [(K_TABLE, "box", origin + TABLE_CENTER, np.eye(3), np.array(TABLE_HALF))]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pts, X, Y, Z = chain(s[Q:Q + 7])
        pts = np.concatenate([pts, [pts[7] + Z * FLANGE_D]]) + origin
        for k in range(8):
            if fin(pts[k], pts[k + 1]):
                out.append((K_ARM0 + k, "capsule", pts[k], pts[k + 1], ARM_RADIUS))
        xh, yh = (X - Y) / np.sqrt(2), (X + Y) / np.sqrt(2)
        G = np.stack([xh, yh, Z])
        tcp = pts[7] + Z * (FLANGE_D + ee_offset_z)
        if fin(G, pts[8]):
            out.append((K_HAND, "box", pts[8] + Z * HAND_CENTER_Z, G, np.array(HAND_HALF)))
        for f in range(2):
            q = s[Q + 7 + f]
            sg = 1.0 if f == 0 else -1.0
            c = tcp + yh * sg * (q + 0.5 * FINGER_THICKNESS) - Z * 0.5 * FINGER_LENGTH
            if fin(G, tcp, q, c):
                out.append((K_FINGER0 + f, "box", c, G, np.array([PAD_HALF_X, 0.5 * FINGER_THICKNESS, PAD_HALF_Z + 0.5 * FINGER_LENGTH])))
        R = quat_to_matrix(s[OBJ_QUAT:OBJ_QUAT + 4])
        c = origin + s[OBJ_POS:OBJ_POS + 3]
        if fin(R, c) and np.linalg.det(R) != 0:
            Gc = np.linalg.inv(R)                      # the cube is the image of [-h, h]^3 under R: local coordinates = R^-1 (x - c)
            if fin(Gc):
                out.append((K_CUBE, "box", c, Gc, np.full(3, CUBE_HALF)))
        g = origin + s[CMD:CMD + 3]
        if draw_targets and fin(g):
            out.append((K_GOAL, "sphere", g, GOAL_RADIUS))
    return out


def box(o, d, c, G, h, near):
    """The box {x : |G_a . (x - c)| <= h_a}: t (M,), normal (M, 3) = the hit face's G row, normalised, facing the ray."""
    ol, dl = (o - c) @ G.T, d @ G.T
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (-h - ol) / dl, (h - ol) / dl
    par = dl == 0
    inside = np.abs(ol) <= h
    lo = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(ta, tb))
    hi = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(ta, tb))
    te, tx = lo.max(1), hi.min(1)
    t, front = vr._pick(te, tx, near)
    a = np.where(front, lo.argmax(1), hi.argmin(1))
    n = G[a] / np.linalg.norm(G[a], axis=1, keepdims=True)
    n = n * np.where((n * d).sum(1) > 0, -1.0, 1.0)[:, None]
    return t, n


def _span_sphere(o, d, c, r):
    oc = o - c
    b, cc = (oc * d).sum(1), (oc * oc).sum(1) - r * r
    disc = b * b - cc
    sq = np.sqrt(np.maximum(disc, 0))
    return np.where(disc >= 0, -b - sq, np.inf), np.where(disc >= 0, -b + sq, -np.inf)


def capsule(o, d, A, B, r, near):
    """The capsule of radius r about the segment A B (A == B: a sphere): t (M,), normal (M, 3) facing the ray.  The ray's span is
    the union of its spans in the two end spheres and in the cylinder between the end planes."""
    a0, a1 = _span_sphere(o, d, A, r)
    b0, b1 = _span_sphere(o, d, B, r)
    t0, t1 = np.minimum(a0, b0), np.maximum(a1, b1)
    ax = B - A
    L = np.linalg.norm(ax)
    oc = o - A
    if L > 0:
        ax = ax / L
        dpar, opar = d @ ax, oc @ ax
        with np.errstate(divide="ignore", invalid="ignore"):
            s0, s1 = -opar / dpar, (L - opar) / dpar
        par = dpar == 0
        ins = (opar >= 0) & (opar <= L)
        sa = np.where(par, np.where(ins, -np.inf, np.inf), np.minimum(s0, s1))
        sb = np.where(par, np.where(ins, np.inf, -np.inf), np.maximum(s0, s1))
        dp, op = d - dpar[:, None] * ax, oc - opar[:, None] * ax
        qa, qb, qc = (dp * dp).sum(1), (op * dp).sum(1), (op * op).sum(1) - r * r
        disc = qb * qb - qa * qc
        with np.errstate(divide="ignore", invalid="ignore"):
            sq = np.sqrt(np.maximum(disc, 0))
            q0, q1 = (-qb - sq) / qa, (-qb + sq) / qa
        zero = qa == 0
        q0 = np.where(zero, np.where(qc <= 0, -np.inf, np.inf), np.where(disc >= 0, q0, np.inf))
        q1 = np.where(zero, np.where(qc <= 0, np.inf, -np.inf), np.where(disc >= 0, q1, -np.inf))
        te, tx = np.maximum(sa, q0), np.minimum(sb, q1)
        ok = te <= tx
        t0, t1 = np.where(ok, np.minimum(t0, te), t0), np.where(ok, np.maximum(t1, tx), t1)
    t, _ = vr._pick(t0, t1, near)
    x = oc + np.where(np.isfinite(t), t, 0)[:, None] * d
    s = np.clip(x @ ax, 0, L) if L > 0 else np.zeros(len(x))
    n = (x - s[:, None] * ax) / r
    n = n * np.where((n * d).sum(1) > 0, -1.0, 1.0)[:, None]
    return t, n


def object_hits(o, d, prims, near, grow=0.0):
    """prims: [(id, kind, params...)] in increasing id order: t (M, P), normals (M, P, 3)."""
    T = np.full((o.shape[0], len(prims)), np.inf)
    Nn = np.zeros((o.shape[0], len(prims), 3))
    for j, pr in enumerate(prims):
        if pr[1] == "box":
            T[:, j], Nn[:, j] = box(o, d, pr[2], pr[3], pr[4] + grow, near)
        elif pr[1] == "capsule":
            T[:, j], Nn[:, j] = capsule(o, d, pr[2], pr[3], pr[4] + grow, near)
        else:
            T[:, j], Nn[:, j] = vr._sphere(o, d, pr[2], pr[3] + grow, near)
    return T, Nn


def render(viewer, state, env_spacing=2.5, ee_offset_z=0.1034, eps=1e-4):
    """The frame of `viewer` (a ViewerCfg) for `state` (N, 64): rgb (H, W, 3) uint8, depth (H, W), id (H, W), gap (H, W) -- the
    distance between the nearest hit and the nearest hit of ANOTHER object -- and graze (H, W): the id changes when every
    primitive grows or shrinks by `eps` metres."""
    W, H = viewer.resolution
    state = np.asarray(state, np.float64)
    n = state.shape[0]
    org = env_origins(n, float(f32(env_spacing)))
    eye = f32(viewer.eye)
    d = vr.camera_rays(eye, f32(viewer.lookat), W, H, viewer.focal_length, viewer.horizontal_aperture).reshape(-1, 3)
    if viewer.origin_type == "env":
        eye = f32(eye + org[viewer.env_index])          # the sum as the kernel's float32 parameter holds it
    o = np.broadcast_to(eye, d.shape).copy()
    near, far = float(f32(viewer.near_clip)), float(f32(viewer.far_clip))
    prims = []
    for e in range(n):
        for pr in primitives(state[e], f32(org[e]), float(f32(ee_offset_z)), viewer.draw_targets):
            prims.append((ID_ENV0 + IDS_PER_ENV * e + pr[0],) + pr[1:])
    ids = np.array([ID_GROUND] + [pr[0] for pr in prims])
    assert (np.diff(ids) > 0).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        tg = (GROUND_Z - o[:, 2]) / d[:, 2]
    tg = np.where((d[:, 2] != 0) & (tg >= near), tg, np.inf)

    def nearest(grow):
        T, Nn = object_hits(o, d, prims, near, grow)
        allT = np.concatenate([tg[:, None], T], 1)
        allT = np.where(allT <= far, allT, np.inf)
        k = np.argmin(allT, 1)                           # ties: the first column = the lower id
        return allT, Nn, k

    allT, Nn, k = nearest(0.0)
    m = np.arange(len(k))
    depth = allT[m, k]
    hit = np.isfinite(depth)
    oid = np.where(hit, ids[k], ID_SKY)
    srt = np.sort(np.concatenate([allT, np.full((len(k), 1), np.inf)], 1), 1)
    with np.errstate(invalid="ignore"):
        gap = np.where(hit, srt[:, 1] - srt[:, 0], np.inf)
    graze = np.zeros(len(k), bool)
    for g in (eps, -eps):
        aT, _, kg = nearest(g)
        graze |= np.where(np.isfinite(aT[m, kg]), ids[kg], ID_SKY) != oid
    nrm = np.zeros((len(k), 3))
    nrm[:] = (0.0, 0.0, 1.0)
    objs = hit & (k > 0)
    nrm[objs] = Nn[m[objs], k[objs] - 1]
    nrm *= np.where((nrm * d).sum(1) > 0, -1.0, 1.0)[:, None]
    alb = np.zeros((len(k), 3))
    alb[oid == ID_GROUND] = ALBEDO["ground"]
    kind = np.where(oid >= ID_ENV0, (oid - ID_ENV0) % IDS_PER_ENV, -1)
    for kk, name in enumerate(KIND_ALBEDO):
        alb[kind == kk] = ALBEDO[name]
    X = o + np.where(hit, depth, 0)[:, None] * d
    L = np.asarray(vr.LIGHT_POS) - X
    L /= np.linalg.norm(L, axis=1, keepdims=True)
    shade = vr.K_AMBIENT + vr.K_DIFFUSE * np.maximum((nrm * L).sum(1), 0.0)
    sky = np.asarray(vr.SKY_HORIZON) + (np.asarray(vr.SKY_ZENITH) - np.asarray(vr.SKY_HORIZON)) * np.maximum(d[:, 2:3], 0.0)
    rgb = np.where(hit[:, None], alb * shade[:, None], sky)
    return (vr._byte(rgb).reshape(H, W, 3), np.where(hit, depth, np.inf).reshape(H, W), oid.reshape(H, W), gap.reshape(H, W),
            graze.reshape(H, W))
