// lift_viewer_kernels.hip -- the rgb_array viewer of FrankaCubeLift-v0 (gfx950): one world-placed pinhole camera that renders every
// env's table, arm, gripper, cube and goal marker into one RGBA image.  DESIGN.md section 37 is the image contract it shares with
// the rover's viewer (camera, hit rule, sky, packing and the host's config code: viewer_common.hpp), section 29 this scene;
// include/rover_lift_viewer.h the ABI.
//
// Reference: ORBIT's RLTaskEnv.render() in "rgb_array" mode (the viewport camera cfg.viewer places; manipulation_env_cfg.py:235
// sets its eye), which gymnasium.wrappers.RecordVideo records in examples/02_train/train.py:123-125.
//
// per frame: a pose pass -- one thread per env runs the modified-DH chain on LIFT_Q and writes the env's world-frame primitives, a
//            bounding sphere and a draw mask into the workspace; an env whose bounds leave the 3 x 3 lattice cells around its own
//            (or the z slab) goes to an overflow list -- then ONE render launch: one wave = one 8 x 8 pixel tile.  The env origins
//            are a regular lattice, so each lane walks the lattice cells its ray crosses inside the z slab with a 2-D DDA and finds
//            the candidate envs by index arithmetic: all nine envs around the first cell, then the three that enter the 3 x 3
//            neighbourhood with every step (no env is tested twice, none whose bounds the ray can reach is left out).  The walk
//            stops when the next cell starts beyond the nearest hit; its trip count is at most rows + cols + 4.
//            Nearest hit wins; equal t goes to the lower object id, so the order of the tests does not matter.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/rover_hip.h"
#include "../../include/rover_lift_viewer.h"
#include "lift_render.hpp"
#include "rover_internal.hpp"
#include "rover_render.hpp"
#include "viewer_common.hpp"

namespace {

using namespace viewer_common;

// ---- per-env record of the pose pass (floats, world frame)
constexpr int PW_SPHERE = 0;    // 4  bounding sphere (centre, radius) of everything the env draws
constexpr int PW_CHAIN = 4;     // 27 base origin, p1 .. p7, flange
constexpr int PW_TCP = 31;      // 3
constexpr int PW_HAND = 34;     // 9  x_hand, y_hand, z_hand
constexpr int PW_FINGER = 43;   // 2  LIFT_Q[7], LIFT_Q[8]
constexpr int PW_CUBE = 45;     // 3  cube centre
constexpr int PW_CUBE_INV = 48; // 9  rows of the inverse of the cube's matrix
constexpr int PW_GOAL = 57;     // 3
constexpr int PW_ORIGIN = 60;   // 3
constexpr int PW_MASK = 63;     // 1  int bits: bit k set = primitive k (0 .. 13) is drawn
constexpr int POSE_WORDS = 64;

// ---- workspace layout: overflow count (256 bytes) | overflow list (n ints) | poses (n x POSE_WORDS floats)
struct Layout {
    size_t off_ovf, off_pose, bytes;
};

Layout layout_of(int n)
{
    Layout L;
    L.off_ovf = 256;
    L.off_pose = align256(L.off_ovf + (size_t)n * sizeof(int));
    L.bytes = align256(L.off_pose + (size_t)n * POSE_WORDS * sizeof(float));
    return L;
}

// rows and cols of the env lattice (the formula of rover_lift_viewer.h)
void lattice_of(int n, int &rows, int &cols)
{
    int r = (int)std::sqrt((double)n);
    while ((long long)r * r > n) --r;
    while ((long long)(r + 1) * (r + 1) <= n) ++r;
    rows = (n + r - 1) / r;
    cols = (n + rows - 1) / rows;
}

struct PoseParams {
    const float *state;
    int n, rows, cols;
    float spacing, inv_spacing;
    float ee_offset_z;
    int draw_targets;
    int *ovf_count, *ovf;
    float *pose;
};

__device__ __forceinline__ bool finite3(const float *a) { return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]); }

struct Bounds {
    float lo[3], hi[3];
};
__device__ __forceinline__ void grow(Bounds &b, const float *c, float r)
{
    for (int i = 0; i < 3; ++i) { b.lo[i] = fminf(b.lo[i], c[i] - r); b.hi[i] = fmaxf(b.hi[i], c[i] + r); }
}

__global__ __launch_bounds__(256) void lift_viewer_pose_kernel(PoseParams p)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= p.n) return;
    constexpr int KIND[7] = LR_KIND;
    constexpr float A[7] = LR_DH_A, D[7] = LR_DH_D;
    const float *S = p.state;
    const size_t N = (size_t)p.n;
    float *o = p.pose + (size_t)env * POSE_WORDS;
    const int row = env / p.cols, col = env % p.cols;
    const float org[3] = {(0.5f * (float)(p.rows - 1) - (float)row) * p.spacing, ((float)col - 0.5f * (float)(p.cols - 1)) * p.spacing, 0.0f};
    int mask = 1 << LR_K_TABLE;
    Bounds bd;
    {
        const float tc[3] = LR_TABLE_CENTER, th[3] = LR_TABLE_HALF;
        for (int i = 0; i < 3; ++i) { bd.lo[i] = org[i] + tc[i] - th[i]; bd.hi[i] = org[i] + tc[i] + th[i]; o[PW_ORIGIN + i] = org[i]; }
    }

    // ---- the arm: frame origins of the modified-DH chain (hand_kinematics of the step), then the flange
    float X[3] = {1.0f, 0.0f, 0.0f}, Y[3] = {0.0f, 1.0f, 0.0f}, Z[3] = {0.0f, 0.0f, 1.0f}, pos[3] = {0.0f, 0.0f, 0.0f};
    float prev[3] = {org[0], org[1], org[2]}, cur[3];
    for (int i = 0; i < 3; ++i) o[PW_CHAIN + i] = prev[i];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const float p0 = A[i], p1 = KIND[i] == 0 ? 0.0f : (KIND[i] > 0 ? -D[i] : D[i]), p2 = KIND[i] == 0 ? D[i] : 0.0f;
        float sn, cs;
        sincosf(S[(LIFT_Q + i) * N + env], &sn, &cs);
        for (int k = 0; k < 3; ++k) {
            pos[k] += X[k] * p0 + Y[k] * p1 + Z[k] * p2;
            cur[k] = org[k] + pos[k];
            o[PW_CHAIN + 3 * (i + 1) + k] = cur[k];
            const float U = KIND[i] == 0 ? Y[k] : (KIND[i] > 0 ? Z[k] : -Z[k]);
            const float Zn = KIND[i] == 0 ? Z[k] : (KIND[i] > 0 ? -Y[k] : Y[k]);
            const float Xn = cs * X[k] + sn * U, Yn = cs * U - sn * X[k];
            X[k] = Xn; Y[k] = Yn; Z[k] = Zn;
        }
        if (finite3(prev) && finite3(cur)) { mask |= 1 << (LR_K_ARM0 + i); grow(bd, prev, LR_ARM_RADIUS); grow(bd, cur, LR_ARM_RADIUS); }
        for (int k = 0; k < 3; ++k) prev[k] = cur[k];
    }
    float tcp[3], xh[3], yh[3];
    const float r2 = 0.70710678118654752f;
    for (int k = 0; k < 3; ++k) {
        cur[k] = org[k] + (pos[k] + Z[k] * LR_FLANGE_D);
        tcp[k] = org[k] + (pos[k] + Z[k] * (LR_FLANGE_D + p.ee_offset_z));
        xh[k] = (X[k] - Y[k]) * r2; yh[k] = (X[k] + Y[k]) * r2;
        o[PW_CHAIN + 24 + k] = cur[k]; o[PW_TCP + k] = tcp[k];
        o[PW_HAND + k] = xh[k]; o[PW_HAND + 3 + k] = yh[k]; o[PW_HAND + 6 + k] = Z[k];
    }
    if (finite3(prev) && finite3(cur)) { mask |= 1 << (LR_K_ARM0 + 7); grow(bd, prev, LR_ARM_RADIUS); grow(bd, cur, LR_ARM_RADIUS); }
    const bool frame_ok = finite3(xh) && finite3(yh) && finite3(Z);
    if (frame_ok && finite3(cur)) {
        const float hh[3] = LR_HAND_HALF;
        float c[3];
        for (int k = 0; k < 3; ++k) c[k] = cur[k] + Z[k] * LR_HAND_CENTER_Z;
        mask |= 1 << LR_K_HAND;
        grow(bd, c, sqrtf(hh[0] * hh[0] + hh[1] * hh[1] + hh[2] * hh[2]));
    }
    for (int f = 0; f < 2; ++f) {
        const float q = S[(LIFT_Q + 7 + f) * N + env];
        o[PW_FINGER + f] = q;
        if (!(frame_ok && finite3(tcp) && isfinite(q))) continue;
        const float sg = f == 0 ? 1.0f : -1.0f, hz = LR_PAD_HALF_Z + 0.5f * LR_FINGER_LENGTH;
        float c[3];
        for (int k = 0; k < 3; ++k) c[k] = tcp[k] + yh[k] * (sg * (q + 0.5f * LR_FINGER_THICKNESS)) - Z[k] * (0.5f * LR_FINGER_LENGTH);
        if (!finite3(c)) continue;
        mask |= 1 << (LR_K_FINGER0 + f);
        grow(bd, c, sqrtf(LR_PAD_HALF_X * LR_PAD_HALF_X + 0.25f * LR_FINGER_THICKNESS * LR_FINGER_THICKNESS + hz * hz));
    }

    // ---- the cube: matrix of the quaternion AS STORED (quat_to_matrix of the step, no normalisation); the box is the image of
    // [-h, h]^3 under it, tested in the coordinates its inverse gives.  A singular matrix spans no volume: not drawn.
    {
        const float w = S[LIFT_OBJ_QUAT * N + env], x = S[(LIFT_OBJ_QUAT + 1) * N + env], y = S[(LIFT_OBJ_QUAT + 2) * N + env],
                    z = S[(LIFT_OBJ_QUAT + 3) * N + env];
        float R[9], c[3], inv[9];
        R[0] = 1.0f - 2.0f * (y * y + z * z); R[1] = 2.0f * (x * y - w * z); R[2] = 2.0f * (x * z + w * y);
        R[3] = 2.0f * (x * y + w * z); R[4] = 1.0f - 2.0f * (x * x + z * z); R[5] = 2.0f * (y * z - w * x);
        R[6] = 2.0f * (x * z - w * y); R[7] = 2.0f * (y * z + w * x); R[8] = 1.0f - 2.0f * (x * x + y * y);
        for (int k = 0; k < 3; ++k) { c[k] = org[k] + S[(LIFT_OBJ_POS + k) * N + env]; o[PW_CUBE + k] = c[k]; }
        const float c00 = R[4] * R[8] - R[5] * R[7], c01 = R[5] * R[6] - R[3] * R[8], c02 = R[3] * R[7] - R[4] * R[6];
        const float det = R[0] * c00 + R[1] * c01 + R[2] * c02, id = 1.0f / det;
        inv[0] = c00 * id; inv[1] = (R[2] * R[7] - R[1] * R[8]) * id; inv[2] = (R[1] * R[5] - R[2] * R[4]) * id;
        inv[3] = c01 * id; inv[4] = (R[0] * R[8] - R[2] * R[6]) * id; inv[5] = (R[2] * R[3] - R[0] * R[5]) * id;
        inv[6] = c02 * id; inv[7] = (R[1] * R[6] - R[0] * R[7]) * id; inv[8] = (R[0] * R[4] - R[1] * R[3]) * id;
        bool ok = finite3(c);
        float ext = 0.0f;
        for (int k = 0; k < 9; ++k) { o[PW_CUBE_INV + k] = inv[k]; ok &= isfinite(inv[k]) && isfinite(R[k]); }
        for (int a = 0; a < 3; ++a) ext += sqrtf(R[a] * R[a] + R[3 + a] * R[3 + a] + R[6 + a] * R[6 + a]);
        ext *= LR_CUBE_HALF;
        if (ok && isfinite(ext)) { mask |= 1 << LR_K_CUBE; grow(bd, c, ext); }
    }
    {
        float c[3];
        for (int k = 0; k < 3; ++k) { c[k] = org[k] + S[(LIFT_CMD + k) * N + env]; o[PW_GOAL + k] = c[k]; }
        if (p.draw_targets && finite3(c)) { mask |= 1 << LR_K_GOAL; grow(bd, c, LR_GOAL_RADIUS); }
    }
    o[PW_MASK] = __int_as_float(mask);

    // ---- bounding sphere about the bounding box, and whether the lattice walk finds this env (else: the overflow list)
    float c[3], h[3];
    for (int k = 0; k < 3; ++k) { c[k] = 0.5f * (bd.lo[k] + bd.hi[k]); h[k] = 0.5f * (bd.hi[k] - bd.lo[k]); }
    float r = sqrtf(dot3(h, h)) * 1.0001f + 1.0e-4f;
    if (!(r < LR_BOUND_MAX && finite3(c))) { c[0] = c[1] = c[2] = 0.0f; r = INFINITY; }
    o[PW_SPHERE] = c[0]; o[PW_SPHERE + 1] = c[1]; o[PW_SPHERE + 2] = c[2]; o[PW_SPHERE + 3] = r;
    // (the box, not the sphere: the sphere about a 1.7 m wide table reaches below the slab)
    const float u_lo = 0.5f * (float)p.rows - bd.hi[0] * p.inv_spacing, u_hi = 0.5f * (float)p.rows - bd.lo[0] * p.inv_spacing;
    const float v_lo = bd.lo[1] * p.inv_spacing + 0.5f * (float)p.cols, v_hi = bd.hi[1] * p.inv_spacing + 0.5f * (float)p.cols;
    const bool regular = isfinite(r) && u_lo >= (float)(row - 1) + LR_CELL_MARGIN && u_hi <= (float)(row + 2) - LR_CELL_MARGIN &&
                         v_lo >= (float)(col - 1) + LR_CELL_MARGIN && v_hi <= (float)(col + 2) - LR_CELL_MARGIN &&
                         bd.lo[2] >= LR_SLAB_Z_LO && bd.hi[2] <= LR_SLAB_Z_HI;
    if (!regular) p.ovf[atomicAdd(p.ovf_count, 1)] = env;          // at most n entries: the list holds them all
}

struct ViewParams {
    int n, rows, cols;
    float inv_spacing;
    const int *ovf_count, *ovf;
    const float *pose;
    Pinhole cam;
    float near_clip, far_clip;
    // outputs
    uint32_t *rgba;
    float *depth;
    int32_t *object_id;
};

// the box {x : |g_a . (x - c)| <= h_a, a = 0, 1, 2}; the normal of face a is g_a, normalised
__device__ void test_box(const float *o, const float *d, const float *c, const float *g, const float *h, float near_clip, float far_clip,
                         int id, Best &b)
{
    const float w[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
    float te = -INFINITY, tx = INFINITY;
    float ne[3] = {0.0f, 0.0f, 0.0f}, nx[3] = {0.0f, 0.0f, 0.0f};     // g of the entry / exit face (selects, no indexed array)
    bool hit = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float ga[3] = {g[3 * a], g[3 * a + 1], g[3 * a + 2]};
        const float ol = dot3(ga, w), dl = dot3(ga, d);
        if (dl == 0.0f) { hit &= fabsf(ol) <= h[a]; continue; }
        const float inv = 1.0f / dl;
        float t0 = (-h[a] - ol) * inv, t1 = (h[a] - ol) * inv;
        if (t0 > t1) { const float x = t0; t0 = t1; t1 = x; }
        if (t0 > te) { te = t0; ne[0] = ga[0]; ne[1] = ga[1]; ne[2] = ga[2]; }
        if (t1 < tx) { tx = t1; nx[0] = ga[0]; nx[1] = ga[1]; nx[2] = ga[2]; }
    }
    if (!(hit && te <= tx)) return;
    const bool front = te >= near_clip;
    const float t = front ? te : tx;
    if (!(t >= near_clip)) return;
    const float ga[3] = {front ? ne[0] : nx[0], front ? ne[1] : nx[1], front ? ne[2] : nx[2]};
    const float nn = 1.0f / sqrtf(dot3(ga, ga));
    const float nrm[3] = {ga[0] * nn, ga[1] * nn, ga[2] * nn};
    offer(b, t, id, nrm, d, far_clip);
}

// the capsule of radius r about the segment A B, given the spans of the ray in the spheres about A and B (shared with the
// neighbouring segments, so coincident end caps give bit-equal t and the lower id wins); A == B is the sphere alone
__device__ void test_capsule(const float *o, const float *d, const float *A, const float *B, float r, bool hit_a, float a0, float a1,
                             bool hit_b, float b0, float b1, float near_clip, float far_clip, int id, Best &b)
{
    float t0 = INFINITY, t1 = -INFINITY;
    if (hit_a) { t0 = a0; t1 = a1; }
    if (hit_b) { t0 = fminf(t0, b0); t1 = fmaxf(t1, b1); }
    float ax[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
    const float l2 = dot3(ax, ax);
    float len = 0.0f;
    const float oc[3] = {o[0] - A[0], o[1] - A[1], o[2] - A[2]};
    if (l2 > 0.0f) {
        len = sqrtf(l2);
        const float il = 1.0f / len;
        for (int i = 0; i < 3; ++i) ax[i] *= il;
        const float dpar = dot3(d, ax), opar = dot3(oc, ax);
        float s0 = -INFINITY, s1 = INFINITY;
        bool hit = true;
        if (dpar == 0.0f) {
            hit = opar >= 0.0f && opar <= len;
        } else {
            const float inv = 1.0f / dpar;
            s0 = -opar * inv; s1 = (len - opar) * inv;
            if (s0 > s1) { const float x = s0; s0 = s1; s1 = x; }
        }
        float dp[3], op[3];
        for (int i = 0; i < 3; ++i) { dp[i] = d[i] - dpar * ax[i]; op[i] = oc[i] - opar * ax[i]; }
        const float qa = dot3(dp, dp), qb = dot3(op, dp), qc = dot3(op, op) - r * r;
        float q0 = -INFINITY, q1 = INFINITY;
        if (qa == 0.0f) {
            hit &= qc <= 0.0f;
        } else {
            const float disc = qb * qb - qa * qc;
            hit &= disc >= 0.0f;
            const float sq = sqrtf(fmaxf(disc, 0.0f));
            q0 = (-qb - sq) / qa; q1 = (-qb + sq) / qa;
        }
        const float te = fmaxf(s0, q0), tx = fminf(s1, q1);
        if (hit && te <= tx) { t0 = fminf(t0, te); t1 = fmaxf(t1, tx); }
    }
    if (!(t0 <= t1)) return;
    const float t = t0 >= near_clip ? t0 : t1;
    if (!(t >= near_clip)) return;
    float x[3], nrm[3];
    for (int i = 0; i < 3; ++i) x[i] = oc[i] + t * d[i];
    const float s = l2 > 0.0f ? fminf(fmaxf(dot3(x, ax), 0.0f), len) : 0.0f;
    const float ir = 1.0f / r;
    for (int i = 0; i < 3; ++i) nrm[i] = (x[i] - s * ax[i]) * ir;
    offer(b, t, id, nrm, d, far_clip);
}

__device__ void test_env(const ViewParams &p, int env, const float *o, const float *d, Best &b)
{
    const float *P = p.pose + (size_t)env * POSE_WORDS;
    {
        float t0, t1;
        if (!sphere_span(o, d, P + PW_SPHERE, P[PW_SPHERE + 3], t0, t1) || t1 < p.near_clip || t0 > b.t) return;
    }
    const int mask = __float_as_int(P[PW_MASK]);
    const int id0 = LR_ID_ENV0 + LR_IDS_PER_ENV * env;
    const float eye3[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    {
        const float tc[3] = LR_TABLE_CENTER, th[3] = LR_TABLE_HALF;
        const float c[3] = {P[PW_ORIGIN] + tc[0], P[PW_ORIGIN + 1] + tc[1], P[PW_ORIGIN + 2] + tc[2]};
        test_box(o, d, c, eye3, th, p.near_clip, p.far_clip, id0 + LR_K_TABLE, b);
    }
    {
        float a0 = 0.0f, a1 = 0.0f, b0 = 0.0f, b1 = 0.0f;
        bool hit_a = sphere_span(o, d, P + PW_CHAIN, LR_ARM_RADIUS, a0, a1);
#pragma unroll 1
        for (int k = 0; k < 8; ++k) {
            const float *A = P + PW_CHAIN + 3 * k, *B = A + 3;
            const bool hit_b = sphere_span(o, d, B, LR_ARM_RADIUS, b0, b1);
            if (mask >> (LR_K_ARM0 + k) & 1)
                test_capsule(o, d, A, B, LR_ARM_RADIUS, hit_a, a0, a1, hit_b, b0, b1, p.near_clip, p.far_clip, id0 + LR_K_ARM0 + k, b);
            hit_a = hit_b; a0 = b0; a1 = b1;
        }
    }
    const float *hand = P + PW_HAND;
    if (mask >> LR_K_HAND & 1) {
        const float hh[3] = LR_HAND_HALF;
        const float *fl = P + PW_CHAIN + 24;
        const float c[3] = {fl[0] + hand[6] * LR_HAND_CENTER_Z, fl[1] + hand[7] * LR_HAND_CENTER_Z, fl[2] + hand[8] * LR_HAND_CENTER_Z};
        test_box(o, d, c, hand, hh, p.near_clip, p.far_clip, id0 + LR_K_HAND, b);
    }
#pragma unroll 1
    for (int f = 0; f < 2; ++f) {
        if (!(mask >> (LR_K_FINGER0 + f) & 1)) continue;
        const float fh[3] = {LR_PAD_HALF_X, 0.5f * LR_FINGER_THICKNESS, LR_PAD_HALF_Z + 0.5f * LR_FINGER_LENGTH};
        const float sy = (f == 0 ? 1.0f : -1.0f) * (P[PW_FINGER + f] + 0.5f * LR_FINGER_THICKNESS), sz = 0.5f * LR_FINGER_LENGTH;
        float c[3];
        for (int i = 0; i < 3; ++i) c[i] = P[PW_TCP + i] + hand[3 + i] * sy - hand[6 + i] * sz;
        test_box(o, d, c, hand, fh, p.near_clip, p.far_clip, id0 + LR_K_FINGER0 + f, b);
    }
    if (mask >> LR_K_CUBE & 1) {
        const float ch[3] = {LR_CUBE_HALF, LR_CUBE_HALF, LR_CUBE_HALF};
        test_box(o, d, P + PW_CUBE, P + PW_CUBE_INV, ch, p.near_clip, p.far_clip, id0 + LR_K_CUBE, b);
    }
    if (mask >> LR_K_GOAL & 1) test_marker(o, d, P + PW_GOAL, LR_GOAL_RADIUS, p.near_clip, p.far_clip, id0 + LR_K_GOAL, b);
}

// the envs of lattice cells (bu + du, bv - 1 .. bv + 1) or (bu - 1 .. bu + 1, bv + dv): one side of a 3 x 3 neighbourhood
__device__ __forceinline__ void test_cell(const ViewParams &p, int cu, int cv, const float *o, const float *d, Best &b)
{
    if (cu < 0 || cv < 0 || cu >= p.rows || cv >= p.cols) return;
    const int env = cu * p.cols + cv;
    if (env < p.n) test_env(p, env, o, d, b);
}

// clip [ts, te] of the ray coordinate go + t gd to [lo, hi]; false: the ray never is inside
__device__ __forceinline__ bool clip_axis(float go, float gd, float lo, float hi, float &ts, float &te)
{
    if (gd == 0.0f) return go >= lo && go <= hi;
    const float ig = 1.0f / gd, a = (lo - go) * ig, c = (hi - go) * ig;
    ts = fmaxf(ts, fminf(a, c)); te = fminf(te, fmaxf(a, c));
    return true;
}

__global__ __launch_bounds__(TILE * TILE * WAVES) void lift_viewer_render_kernel(ViewParams p)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    if (wave >= p.cam.tiles) return;
    const int lane = threadIdx.x & 63;
    const int u = (wave % p.cam.tiles_x) * TILE + (lane & (TILE - 1));
    const int v = (wave / p.cam.tiles_x) * TILE + (lane >> 3);
    if (u >= p.cam.img_w || v >= p.cam.img_h) return;

    // ---- ray through the pixel centre
    const float o[3] = {p.cam.eye[0], p.cam.eye[1], p.cam.eye[2]};
    const float cx = ((float)u + 0.5f - p.cam.half_w) * p.cam.inv_f, cy = -((float)v + 0.5f - p.cam.half_h) * p.cam.inv_f;
    float d[3];
    for (int i = 0; i < 3; ++i) d[i] = p.cam.fwd[i] + cx * p.cam.right[i] + cy * p.cam.up[i];
    const float dn = 1.0f / sqrtf(dot3(d, d));
    for (int i = 0; i < 3; ++i) d[i] *= dn;

    // ---- ground plane
    Best b;
    b.t = INFINITY; b.id = LR_ID_SKY; b.n[0] = b.n[1] = b.n[2] = 0.0f;
    if (d[2] != 0.0f) {
        const float t = (LR_GROUND_Z - o[2]) / d[2];
        const float up[3] = {0.0f, 0.0f, 1.0f};
        if (t >= p.near_clip) offer(b, t, LR_ID_GROUND, up, d, p.far_clip);
    }

    // ---- the overflow list, then the lattice walk
    const int n_ovf = *p.ovf_count;
    for (int k = 0; k < n_ovf; ++k) test_env(p, p.ovf[k], o, d, b);
    {
        // lattice coordinates: row axis gu = rows / 2 - x / spacing, column axis gv = y / spacing + cols / 2; cell = floor
        const float gou = 0.5f * (float)p.rows - o[0] * p.inv_spacing, gdu = -d[0] * p.inv_spacing;
        const float gov = o[1] * p.inv_spacing + 0.5f * (float)p.cols, gdv = d[1] * p.inv_spacing;
        float ts = p.near_clip, te = p.far_clip;
        bool walk = clip_axis(gou, gdu, -1.0f, (float)(p.rows + 1), ts, te);
        walk &= clip_axis(gov, gdv, -1.0f, (float)(p.cols + 1), ts, te);
        walk &= clip_axis(o[2], d[2], LR_SLAB_Z_LO, LR_SLAB_Z_HI, ts, te);
        walk &= ts <= te && ts <= b.t;
        if (walk) {
            const int su = gdu > 0.0f ? 1 : -1, sv = gdv > 0.0f ? 1 : -1;
            const float igu = gdu == 0.0f ? 0.0f : 1.0f / gdu, igv = gdv == 0.0f ? 0.0f : 1.0f / gdv;
            int bu = min(max((int)floorf(fmaf(ts, gdu, gou)), -1), p.rows);
            int bv = min(max((int)floorf(fmaf(ts, gdv, gov)), -1), p.cols);
            for (int i = -1; i <= 1; ++i)
                for (int j = -1; j <= 1; ++j) test_cell(p, bu + i, bv + j, o, d, b);
            for (;;) {
                const float tnu = gdu == 0.0f ? INFINITY : ((float)(bu + (su > 0)) - gou) * igu;
                const float tnv = gdv == 0.0f ? INFINITY : ((float)(bv + (sv > 0)) - gov) * igv;
                if (!(fminf(tnu, tnv) <= fminf(te, b.t))) break;
                if (tnu <= tnv) {
                    bu += su;
                    if (bu < -1 || bu > p.rows) break;
                    for (int j = -1; j <= 1; ++j) test_cell(p, bu + su, bv + j, o, d, b);
                } else {
                    bv += sv;
                    if (bv < -1 || bv > p.cols) break;
                    for (int i = -1; i <= 1; ++i) test_cell(p, bu + i, bv + sv, o, d, b);
                }
            }
        }
    }

    // ---- shading
    float rgb[3];
    if (b.id == LR_ID_SKY) {
        sky_colour(d, rgb);
    } else {
        const int kind = b.id < LR_ID_ENV0 ? -1 : (b.id - LR_ID_ENV0) % LR_IDS_PER_ENV;
        const float gr[3] = LR_ALBEDO_GROUND, tb[3] = LR_ALBEDO_TABLE, ar[3] = LR_ALBEDO_ARM, hd[3] = LR_ALBEDO_HAND,
                    fg[3] = LR_ALBEDO_FINGER, cb[3] = LR_ALBEDO_CUBE, gl[3] = LR_ALBEDO_GOAL;
        const float lp[3] = RR_LIGHT_POS;
        float l[3];
        for (int i = 0; i < 3; ++i) l[i] = lp[i] - (o[i] + b.t * d[i]);
        const float ln = 1.0f / sqrtf(dot3(l, l));
        const float shade = RR_K_AMBIENT + RR_K_DIFFUSE * fmaxf(dot3(b.n, l) * ln, 0.0f);
        for (int i = 0; i < 3; ++i) {
            const float alb = kind < 0 ? gr[i] : kind == LR_K_TABLE ? tb[i] : kind < LR_K_HAND ? ar[i] : kind == LR_K_HAND ? hd[i]
                              : kind < LR_K_CUBE ? fg[i] : kind == LR_K_CUBE ? cb[i] : gl[i];
            rgb[i] = alb * shade;
        }
    }
    const size_t px = (size_t)v * p.cam.img_w + u;
    p.rgba[px] = pack_rgba(rgb);
    if (p.depth) p.depth[px] = b.id == LR_ID_SKY ? INFINITY : b.t;
    if (p.object_id) p.object_id[px] = b.id;
}

// the C entry's checks: the shared ones, then the lift's two members
bool config_ok(const rover_lift_viewer_config *c, int n)
{
    return view_config_ok(c, n) && std::isfinite(c->env_spacing) && c->env_spacing > 0.0f && std::isfinite(c->ee_offset_z);
}

void origin_of(int env, int rows, int cols, double spacing, double *out)
{
    const int row = env / cols, col = env % cols;
    out[0] = (0.5 * (rows - 1) - row) * spacing;
    out[1] = (col - 0.5 * (cols - 1)) * spacing;
    out[2] = 0.0;
}

}  // namespace

extern "C" {

int rover_lift_viewer_default_config(rover_lift_viewer_config *c)
{
    if (!c) return rover_internal_fail(ROVER_ERR_INVALID, "cfg is NULL");
    default_view(c, -6.0f, -6.0f, 3.5f);                       // manipulation_env_cfg.py:235
    c->env_spacing = 2.5f;
    c->ee_offset_z = 0.1034f;
    return ROVER_OK;
}

size_t rover_lift_viewer_config_bytes(void) { return sizeof(rover_lift_viewer_config); }

size_t rover_lift_viewer_workspace_bytes(int32_t num_envs, const rover_lift_viewer_config *cfg)
{
    if (num_envs <= 0 || !config_ok(cfg, num_envs)) return 0;
    return layout_of(num_envs).bytes;
}

int rover_lift_viewer_constants(float *out, int32_t cap)
{
    constexpr int KIND[7] = LR_KIND;
    constexpr float A[7] = LR_DH_A, D[7] = LR_DH_D;
    float t[25];
    int n = 0;
    for (int i = 0; i < 7; ++i) { t[n++] = (float)KIND[i]; t[n++] = A[i]; t[n++] = D[i]; }
    t[n++] = LR_FLANGE_D; t[n++] = LR_CUBE_HALF; t[n++] = LR_PAD_HALF_X; t[n++] = LR_PAD_HALF_Z;
    if (out) for (int i = 0; i < n && i < cap; ++i) out[i] = t[i];
    return n;
}

int rover_lift_viewer_env_origins(int32_t num_envs, float env_spacing, float *out_host)
{
    if (num_envs <= 0 || !out_host || !std::isfinite(env_spacing)) return rover_internal_fail(ROVER_ERR_INVALID, "num_envs <= 0, out is NULL or env_spacing is not finite");
    int rows, cols;
    lattice_of(num_envs, rows, cols);
    for (int e = 0; e < num_envs; ++e) {
        double o[3];
        origin_of(e, rows, cols, (double)env_spacing, o);
        for (int i = 0; i < 3; ++i) out_host[3 * (size_t)e + i] = (float)o[i];
    }
    return ROVER_OK;
}

int rover_lift_viewer_render(const float *state, int32_t num_envs, const rover_lift_viewer_config *cfg, void *ws, size_t ws_bytes,
                             uint32_t *rgba, float *depth, int32_t *object_id, void *stream)
{
    if (!state || !ws || !rgba) return rover_internal_fail(ROVER_ERR_INVALID, "state / ws / rgba is NULL");
    if (num_envs <= 0) return rover_internal_fail(ROVER_ERR_INVALID, "num_envs must be >= 1");
    if (!config_ok(cfg, num_envs)) return rover_internal_fail(ROVER_ERR_INVALID, "invalid rover_lift_viewer_config");
    const Layout L = layout_of(num_envs);
    if (ws_bytes < L.bytes) return rover_internal_fail(ROVER_ERR_INVALID, "lift viewer workspace too small");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return rover_internal_fail(ROVER_ERR_INVALID, "lift viewer workspace must be 256-byte aligned");
    int dev = 0;
    if (int rc = device_of(state, &dev, true)) return rc;
    {
        hipPointerAttribute_t at;                                  // a plain host pointer may come back as "unregistered"
        if (hipPointerGetAttributes(&at, state) != hipSuccess || at.type != hipMemoryTypeDevice) {
            (void)hipGetLastError();
            return rover_internal_fail(ROVER_ERR_INVALID, "state is not device memory");
        }
    }
    DeviceGuard guard(dev);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *base = static_cast<char *>(ws);
    int rows, cols;
    lattice_of(num_envs, rows, cols);

    PoseParams pp;
    pp.state = state; pp.n = num_envs; pp.rows = rows; pp.cols = cols;
    pp.spacing = cfg->env_spacing; pp.inv_spacing = 1.0f / cfg->env_spacing;
    pp.ee_offset_z = cfg->ee_offset_z; pp.draw_targets = cfg->draw_targets != 0;
    pp.ovf_count = reinterpret_cast<int *>(base);
    pp.ovf = reinterpret_cast<int *>(base + L.off_ovf);
    pp.pose = reinterpret_cast<float *>(base + L.off_pose);
    HIP_TRY(hipMemsetAsync(pp.ovf_count, 0, sizeof(int), st));
    hipLaunchKernelGGL(lift_viewer_pose_kernel, dim3((unsigned)((num_envs + 255) / 256)), dim3(256), 0, st, pp);

    ViewParams p;
    p.n = num_envs; p.rows = rows; p.cols = cols; p.inv_spacing = pp.inv_spacing;
    p.ovf_count = pp.ovf_count; p.ovf = pp.ovf; p.pose = pp.pose;
    double org[3] = {0.0, 0.0, 0.0};
    if (cfg->origin_type == ROVER_VIEWER_ORIGIN_ENV) origin_of(cfg->env_index, rows, cols, (double)cfg->env_spacing, org);
    p.cam = pinhole_of(cfg, org);
    p.near_clip = cfg->near_clip; p.far_clip = cfg->far_clip;
    p.rgba = rgba; p.depth = depth; p.object_id = object_id;
    const unsigned blocks = (unsigned)((p.cam.tiles + WAVES - 1) / WAVES);
    hipLaunchKernelGGL(lift_viewer_render_kernel, dim3(blocks), dim3(TILE * TILE * WAVES), 0, st, p);
    HIP_TRY(hipGetLastError());
    return ROVER_OK;
}

}  // extern "C"
