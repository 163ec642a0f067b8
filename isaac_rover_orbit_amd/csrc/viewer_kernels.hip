// viewer_kernels.hip -- the rgb_array viewer (gfx950): one world-placed pinhole camera that renders the terrain mesh, every env's
// rover and every env's target into one RGBA image.  DESIGN.md section 37 is the image contract it shares with the lift's viewer
// (camera, hit rule, sky, packing and the host's config code: viewer_common.hpp), section 11 this scene; include/rover_viewer.h the ABI.
//
// Reference: ORBIT's RLTaskEnv.render() in "rgb_array" mode (the viewport camera cfg.viewer places; rover_env_cfg.py:272 sets its
// eye), which gymnasium.wrappers.RecordVideo records in examples/02_train/train.py:123-125.
//
// prepare:   the camera's max-height pyramid of the terrain (rover_internal_build_pyramid, camera_kernels.hip).
// per frame: a binning pass -- a counting sort of the rovers' and targets' bounding spheres into the pyramid's 64 x 64-cell
//            blocks (count, exclusive scan, scatter; an item whose bounds leave the terrain's x-y extent goes to an overflow list
//            every ray tests) -- then ONE render launch: one wave = one 8 x 8 pixel tile.  Each lane marches its ray over the
//            terrain (terrain_march.hpp, the camera's march), then walks the coarse blocks its ray crosses up to the nearest hit
//            so far and tests the items binned there.  This walk is separate from the terrain march, so the march's block skip
//            (which skips a block while the ray is above the block's TERRAIN maximum) cannot skip a rover standing on that block.
//            Nearest hit wins; equal t goes to the lower object id, so the binning order does not matter.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/rover_hip.h"
#include "../../include/rover_viewer.h"
#include "rover_internal.hpp"
#include "rover_model.hpp"
#include "rover_render.hpp"
#include "terrain_march.hpp"
#include "viewer_common.hpp"

namespace {

using namespace viewer_common;

using terrain_march::L2;
using terrain_march::Pyramid;
using terrain_march::pyramid_of;

constexpr int POSE_WORDS = 48;  // per env: pos (3), R row-major (9), wheel centres (6 x 3), wheel axles (6 x 3), world frame

// ---- workspace layout (all offsets 256-byte aligned): pyramid | counts | start | cursor | items | overflow | poses
struct Layout {
    Pyramid py;
    int nb;                      // coarse blocks (pyramid level 2)
    int kspan;                   // coarse blocks an item's bounds can cover along one axis
    size_t n_items, cap;         // 2 per env (rover, target); bin entries
    size_t off_cnt, off_start, off_cur, off_items, off_ovf, off_pose, bytes;
    float rover_r;               // bounding radius of a rover about its root position (any bogie / steer angle)
};

float rover_bound_radius()
{
    const float wheel[6][3] = RV_WHEEL_B_INIT, pivot[3][3] = RV_BOGIE_PIVOT_INIT;
    const int bog[6] = RV_WHEEL_BOGIE_INIT;
    const float cc[3] = RR_CHASSIS_CENTER, ch[3] = RR_CHASSIS_HALF;
    const double rim = std::sqrt((double)RV_WHEEL_CONTACT_RADIUS * RV_WHEEL_CONTACT_RADIUS +
                                 (double)RR_WHEEL_HALF_WIDTH * RR_WHEEL_HALF_WIDTH);
    double c[3] = {cc[0], cc[1], cc[2]}, h[3] = {ch[0], ch[1], ch[2]};
    double r = norm3(c) + norm3(h);
    for (int k = 0; k < 6; ++k) {
        const float *P = pivot[bog[k]];
        const double p[3] = {P[0], P[1], P[2]}, d[3] = {wheel[k][0] - P[0], wheel[k][1] - P[1], wheel[k][2] - P[2]};
        r = std::fmax(r, norm3(p) + norm3(d) + rim);
    }
    return (float)(r * 1.001 + 1.0e-3);
}

Layout layout_of(const rover_sim_view &s)
{
    Layout L;
    L.py = pyramid_of(s.H, s.W);
    L.nb = L.py.c2x * L.py.c2y;
    L.rover_r = rover_bound_radius();
    const double rmax = std::fmax((double)L.rover_r, (double)RR_TARGET_RADIUS);
    const double span = 2.0 * rmax / s.res + 2.0;                 // cells, with the one-cell pad on each side
    L.kspan = (int)std::floor(span / L2) + 2;
    L.n_items = 2 * (size_t)s.n;
    L.cap = L.n_items * (size_t)L.kspan * (size_t)L.kspan;
    L.off_cnt = align256(L.py.bytes);
    L.off_start = align256(L.off_cnt + (size_t)(L.nb + 1) * sizeof(int));
    L.off_cur = align256(L.off_start + (size_t)(L.nb + 1) * sizeof(int));
    L.off_items = align256(L.off_cur + (size_t)L.nb * sizeof(int));
    L.off_ovf = align256(L.off_items + L.cap * sizeof(int));
    L.off_pose = align256(L.off_ovf + L.n_items * sizeof(int));
    L.bytes = align256(L.off_pose + (size_t)s.n * POSE_WORDS * sizeof(float));
    return L;
}

struct BinParams {
    const float *state;
    int n;
    int W, H, c2x, c2y;
    float inv_res, min_x, min_y;
    float rover_r;
    int draw_targets;
    int *counts;                 // [nb] per block, [nb] = overflow count
    int *start, *cursor, *items, *ovf;
    float *pose;
};

// bounding sphere of item `it` (env = it >> 1; kind 0 rover, 1 target)
__device__ __forceinline__ void item_sphere(const BinParams &p, int it, float &cx, float &cy, float &r)
{
    const size_t N = (size_t)p.n, env = (size_t)(it >> 1);
    if ((it & 1) == 0) {
        cx = p.state[ROVER_POS * N + env]; cy = p.state[(ROVER_POS + 1) * N + env]; r = p.rover_r;
    } else {
        cx = p.state[ROVER_TARGET_W * N + env]; cy = p.state[(ROVER_TARGET_W + 1) * N + env]; r = RR_TARGET_RADIUS;
    }
}

// the coarse blocks an item's bounds (padded by one cell) cover; false: the bounds leave the terrain (or are not finite)
__device__ __forceinline__ bool item_blocks(const BinParams &p, int it, int &bx0, int &bx1, int &by0, int &by1)
{
    float cx, cy, r;
    item_sphere(p, it, cx, cy, r);
    const float gx0 = (cx - r - p.min_x) * p.inv_res - 1.0f, gx1 = (cx + r - p.min_x) * p.inv_res + 1.0f;
    const float gy0 = (cy - r - p.min_y) * p.inv_res - 1.0f, gy1 = (cy + r - p.min_y) * p.inv_res + 1.0f;
    if (!(gx0 >= 0.0f && gx1 <= (float)(p.W - 1) && gy0 >= 0.0f && gy1 <= (float)(p.H - 1))) return false;
    bx0 = min((int)(gx0 * (1.0f / L2)), p.c2x - 1); bx1 = min((int)(gx1 * (1.0f / L2)), p.c2x - 1);
    by0 = min((int)(gy0 * (1.0f / L2)), p.c2y - 1); by1 = min((int)(gy1 * (1.0f / L2)), p.c2y - 1);
    return true;
}

__device__ __forceinline__ void rot_axis(const float *ax, float s, float c, const float *v, float *out)
{
    const float ad = ax[0] * v[0] + ax[1] * v[1] + ax[2] * v[2];
    const float x[3] = {ax[1] * v[2] - ax[2] * v[1], ax[2] * v[0] - ax[0] * v[2], ax[0] * v[1] - ax[1] * v[0]};
    for (int i = 0; i < 3; ++i) out[i] = v[i] * c + x[i] * s + ax[i] * ad * (1.0f - c);
}

// the world pose of env `env`'s chassis and wheels from its state words (model kinematics, rover_model.hpp)
__device__ void write_pose(const BinParams &p, int env)
{
    const float wheel[6][3] = RV_WHEEL_B_INIT, pivot[3][3] = RV_BOGIE_PIVOT_INIT, axis[3][3] = RV_BOGIE_AXIS_INIT;
    const int bog[6] = RV_WHEEL_BOGIE_INIT, steer[6] = RV_WHEEL_STEER_INIT;
    const float *S = p.state;
    const size_t N = (size_t)p.n;
    float *o = p.pose + (size_t)env * POSE_WORDS;
    float qw = S[ROVER_QUAT * N + env], qx = S[(ROVER_QUAT + 1) * N + env], qy = S[(ROVER_QUAT + 2) * N + env], qz = S[(ROVER_QUAT + 3) * N + env];
    const float qn = 1.0f / sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
    qw *= qn; qx *= qn; qy *= qn; qz *= qn;
    float R[9];
    R[0] = 1.0f - 2.0f * (qy * qy + qz * qz); R[1] = 2.0f * (qx * qy - qw * qz); R[2] = 2.0f * (qx * qz + qw * qy);
    R[3] = 2.0f * (qx * qy + qw * qz); R[4] = 1.0f - 2.0f * (qx * qx + qz * qz); R[5] = 2.0f * (qy * qz - qw * qx);
    R[6] = 2.0f * (qx * qz - qw * qy); R[7] = 2.0f * (qy * qz + qw * qx); R[8] = 1.0f - 2.0f * (qx * qx + qy * qy);
    float pos[3];
    for (int i = 0; i < 3; ++i) { pos[i] = S[(ROVER_POS + i) * N + env]; o[i] = pos[i]; }
    for (int i = 0; i < 9; ++i) o[3 + i] = R[i];
    float bs[3], bc[3];
    for (int j = 0; j < 3; ++j) sincosf(S[(ROVER_BOGIE_Q + j) * N + env], &bs[j], &bc[j]);
    for (int k = 0; k < 6; ++k) {
        const int j = bog[k];
        const float d[3] = {wheel[k][0] - pivot[j][0], wheel[k][1] - pivot[j][1], wheel[k][2] - pivot[j][2]};
        float cb[3], ab[3], a0[3] = {0.0f, 1.0f, 0.0f};           // drive axis at zero steer: Body +Y
        rot_axis(axis[j], bs[j], bc[j], d, cb);
        for (int i = 0; i < 3; ++i) cb[i] += pivot[j][i];
        if (steer[k] >= 0) {                                      // steer axis Body +Z (rover_model.json steer_axis)
            float ss, sc;
            sincosf(S[(ROVER_STEER_Q + steer[k]) * N + env], &ss, &sc);
            a0[0] = -ss; a0[1] = sc;
        }
        rot_axis(axis[j], bs[j], bc[j], a0, ab);
        for (int i = 0; i < 3; ++i) {
            o[12 + 3 * k + i] = pos[i] + R[3 * i] * cb[0] + R[3 * i + 1] * cb[1] + R[3 * i + 2] * cb[2];
            o[30 + 3 * k + i] = R[3 * i] * ab[0] + R[3 * i + 1] * ab[1] + R[3 * i + 2] * ab[2];
        }
    }
}

__global__ __launch_bounds__(256) void viewer_bin_count_kernel(BinParams p)
{
    const int it = blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= 2 * p.n) return;
    if ((it & 1) == 0) write_pose(p, it >> 1);
    else if (!p.draw_targets) return;
    int bx0, bx1, by0, by1;
    const int nb = p.c2x * p.c2y;
    if (!item_blocks(p, it, bx0, bx1, by0, by1)) {
        p.ovf[atomicAdd(p.counts + nb, 1)] = it;                   // at most 2 n items: the list holds them all
        return;
    }
    for (int by = by0; by <= by1; ++by)
        for (int bx = bx0; bx <= bx1; ++bx) atomicAdd(p.counts + by * p.c2x + bx, 1);
}

// exclusive scan of the nb block counts into start[0 .. nb] and cursor[0 .. nb); one workgroup of 256
__global__ __launch_bounds__(256) void viewer_bin_scan_kernel(BinParams p)
{
    __shared__ int part[256];
    const int nb = p.c2x * p.c2y, t = threadIdx.x;
    const int chunk = (nb + 255) / 256;
    const int i0 = min(t * chunk, nb), i1 = min(i0 + chunk, nb);
    int s = 0;
    for (int i = i0; i < i1; ++i) s += p.counts[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {                      // inclusive Hillis-Steele scan of the 256 partial sums
        const int v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int i = i0; i < i1; ++i) {
        p.start[i] = run;
        p.cursor[i] = run;
        run += p.counts[i];
    }
    if (t == 255) p.start[nb] = part[255];
}

__global__ __launch_bounds__(256) void viewer_bin_scatter_kernel(BinParams p)
{
    const int it = blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= 2 * p.n || ((it & 1) && !p.draw_targets)) return;
    int bx0, bx1, by0, by1;
    if (!item_blocks(p, it, bx0, bx1, by0, by1)) return;
    for (int by = by0; by <= by1; ++by)
        for (int bx = bx0; bx <= bx1; ++bx) p.items[atomicAdd(p.cursor + by * p.c2x + bx, 1)] = it;
}

struct ViewParams {
    // terrain and pyramid (the names march_terrain reads)
    const float *height, *obstacle;
    const float *l1, *l2, *zmax;
    int H, W, c1x, c2x, c2y;
    float inv_res, min_x, min_y;
    // rovers and targets
    const float *state;
    int n;
    int origin_env;              // -1: world origin
    int draw_targets;
    const int *start, *items, *ovf_count, *ovf;
    const float *pose;
    float rover_r;
    Pinhole cam;
    float near_clip, far_clip;
    // outputs
    uint32_t *rgba;
    float *depth;
    int32_t *object_id;
};

__device__ void test_target(const ViewParams &p, int env, const float *o, const float *d, float near_clip, Best &b)
{
    const size_t N = (size_t)p.n;
    const float c[3] = {p.state[ROVER_TARGET_W * N + env], p.state[(ROVER_TARGET_W + 1) * N + env],
                        p.state[(ROVER_TARGET_W + 2) * N + env] + RR_TARGET_Z_OFFSET};
    test_marker(o, d, c, RR_TARGET_RADIUS, near_clip, p.far_clip, RR_ID_ENV0 + RR_IDS_PER_ENV * env + 7, b);
}

__device__ void test_rover(const ViewParams &p, int env, const float *o, const float *d, float near_clip, Best &b)
{
    const float *P = p.pose + (size_t)env * POSE_WORDS;
    {   // bounding sphere about the root position
        float t0, t1;
        if (!sphere_span(o, d, P, p.rover_r, t0, t1) || t1 < near_clip || t0 > b.t) return;
    }
    const int id0 = RR_ID_ENV0 + RR_IDS_PER_ENV * env;
    const float *R = P + 3;
    {   // chassis box, in the Body frame: o' = R^T (o - pos), d' = R^T d
        const float cc[3] = RR_CHASSIS_CENTER, hh[3] = RR_CHASSIS_HALF;
        const float w[3] = {o[0] - P[0], o[1] - P[1], o[2] - P[2]};
        float te = -INFINITY, tx = INFINITY, dl[3];
        int ae = 0, ax = 0;
        bool hit = true;
        for (int a = 0; a < 3; ++a) {
            const float ol = R[a] * w[0] + R[3 + a] * w[1] + R[6 + a] * w[2] - cc[a];
            dl[a] = R[a] * d[0] + R[3 + a] * d[1] + R[6 + a] * d[2];
            if (dl[a] == 0.0f) { hit &= fabsf(ol) <= hh[a]; continue; }
            const float inv = 1.0f / dl[a];
            float t0 = (-hh[a] - ol) * inv, t1 = (hh[a] - ol) * inv;
            if (t0 > t1) { const float x = t0; t0 = t1; t1 = x; }
            if (t0 > te) { te = t0; ae = a; }
            if (t1 < tx) { tx = t1; ax = a; }
        }
        if (hit && te <= tx) {
            const bool front = te >= near_clip;
            const float t = front ? te : tx;
            const int a = front ? ae : ax;
            if (t >= near_clip) {
                const float nrm[3] = {R[a], R[3 + a], R[6 + a]};  // the face normal, Body axis a -> world column a (nrm . d is dl[a])
                offer(b, t, id0, nrm, d, p.far_clip);
            }
        }
    }
    for (int k = 0; k < 6; ++k) {   // wheels: finite cylinders
        const float *c = P + 12 + 3 * k, *ax = P + 30 + 3 * k;
        const float oc[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
        const float dpar = dot3(d, ax), opar = dot3(oc, ax);
        float s0 = -INFINITY, s1 = INFINITY;
        if (dpar == 0.0f) {
            if (fabsf(opar) > RR_WHEEL_HALF_WIDTH) continue;
        } else {
            const float inv = 1.0f / dpar;
            s0 = (-RR_WHEEL_HALF_WIDTH - opar) * inv; s1 = (RR_WHEEL_HALF_WIDTH - opar) * inv;
            if (s0 > s1) { const float x = s0; s0 = s1; s1 = x; }
        }
        float dp[3], op[3];
        for (int i = 0; i < 3; ++i) { dp[i] = d[i] - dpar * ax[i]; op[i] = oc[i] - opar * ax[i]; }
        const float A = dot3(dp, dp), B = dot3(op, dp), Cc = dot3(op, op) - RV_WHEEL_CONTACT_RADIUS * RV_WHEEL_CONTACT_RADIUS;
        float q0 = -INFINITY, q1 = INFINITY;
        if (A == 0.0f) {
            if (Cc > 0.0f) continue;
        } else {
            const float disc = B * B - A * Cc;
            if (!(disc >= 0.0f)) continue;
            const float sq = sqrtf(disc);
            q0 = (-B - sq) / A; q1 = (-B + sq) / A;
        }
        const float te = fmaxf(s0, q0), tx = fminf(s1, q1);
        if (!(te <= tx)) continue;
        const bool front = te >= near_clip;
        const float t = front ? te : tx;
        if (!(t >= near_clip)) continue;
        const bool cap = front ? s0 > q0 : s1 < q1;
        float nrm[3];
        if (cap) {
            for (int i = 0; i < 3; ++i) nrm[i] = ax[i];
        } else {
            float x[3];
            for (int i = 0; i < 3; ++i) x[i] = oc[i] + t * d[i];
            const float xp = dot3(x, ax);
            for (int i = 0; i < 3; ++i) nrm[i] = x[i] - xp * ax[i];
            const float nn = 1.0f / sqrtf(fmaxf(dot3(nrm, nrm), 1.0e-30f));
            for (int i = 0; i < 3; ++i) nrm[i] *= nn;
        }
        offer(b, t, id0 + 1 + k, nrm, d, p.far_clip);
    }
}

__device__ __forceinline__ void test_item(const ViewParams &p, int it, const float *o, const float *d, Best &b)
{
    if (it & 1) test_target(p, it >> 1, o, d, p.near_clip, b);
    else test_rover(p, it >> 1, o, d, p.near_clip, b);
}

__global__ __launch_bounds__(TILE * TILE * WAVES) void rover_viewer_render_kernel(ViewParams p)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    if (wave >= p.cam.tiles) return;
    const int lane = threadIdx.x & 63;
    const int u = (wave % p.cam.tiles_x) * TILE + (lane & (TILE - 1));
    const int v = (wave / p.cam.tiles_x) * TILE + (lane >> 3);
    if (u >= p.cam.img_w || v >= p.cam.img_h) return;

    // ---- eye (wave-uniform), ray through the pixel centre
    float o[3] = {p.cam.eye[0], p.cam.eye[1], p.cam.eye[2]};
    if (p.origin_env >= 0) {
        const size_t N = (size_t)p.n;
        for (int i = 0; i < 3; ++i) o[i] += p.state[(ROVER_POS + i) * N + p.origin_env];
    }
    const float cx = ((float)u + 0.5f - p.cam.half_w) * p.cam.inv_f, cy = -((float)v + 0.5f - p.cam.half_h) * p.cam.inv_f;
    float d[3];
    for (int i = 0; i < 3; ++i) d[i] = p.cam.fwd[i] + cx * p.cam.right[i] + cy * p.cam.up[i];
    const float dn = 1.0f / sqrtf(dot3(d, d));
    for (int i = 0; i < 3; ++i) d[i] *= dn;

    // ---- terrain
    terrain_march::MarchHit mh;
    Best b;
    b.t = terrain_march::march_terrain<true>(p, o[0], o[1], o[2], d[0], d[1], d[2], mh);
    b.id = isfinite(b.t) ? RR_ID_GROUND : RR_ID_SKY;
    b.n[0] = b.n[1] = b.n[2] = 0.0f;

    // ---- rovers and targets: the overflow list, then the bins of the coarse blocks the ray crosses before its nearest hit
    const int n_ovf = *p.ovf_count;
    for (int k = 0; k < n_ovf; ++k) test_item(p, p.ovf[k], o, d, b);
    {
        const float gox = (o[0] - p.min_x) * p.inv_res, goy = (o[1] - p.min_y) * p.inv_res;
        const float gdx = d[0] * p.inv_res, gdy = d[1] * p.inv_res;
        const bool parx = gdx == 0.0f, pary = gdy == 0.0f;
        const float igx = parx ? 0.0f : 1.0f / gdx, igy = pary ? 0.0f : 1.0f / gdy;
        const float xmax = (float)(p.W - 1), ymax = (float)(p.H - 1);
        float ts = p.near_clip, te = p.far_clip;
        bool walk = isfinite(gox) && isfinite(goy);
        if (parx) walk &= gox >= 0.0f && gox <= xmax;
        else { const float a = -gox * igx, c = (xmax - gox) * igx; ts = fmaxf(ts, fminf(a, c)); te = fminf(te, fmaxf(a, c)); }
        if (pary) walk &= goy >= 0.0f && goy <= ymax;
        else { const float a = -goy * igy, c = (ymax - goy) * igy; ts = fmaxf(ts, fminf(a, c)); te = fminf(te, fmaxf(a, c)); }
        walk &= ts <= te && ts <= b.t;
        if (walk) {
            const int sx = gdx > 0.0f ? 1 : -1, sy = gdy > 0.0f ? 1 : -1;
            const int ux = sx > 0, uy = sy > 0;
            int bx = min(max((int)floorf(fmaf(ts, gdx, gox) * (1.0f / L2)), 0), p.c2x - 1);
            int by = min(max((int)floorf(fmaf(ts, gdy, goy) * (1.0f / L2)), 0), p.c2y - 1);
            for (;;) {
                const int blk = by * p.c2x + bx;
                const int k1 = p.start[blk + 1];
                for (int k = p.start[blk]; k < k1; ++k) test_item(p, p.items[k], o, d, b);
                const float tnx = terrain_march::lo_boundary_t((float)((bx + ux) * L2), gox, igx, parx);
                const float tny = terrain_march::lo_boundary_t((float)((by + uy) * L2), goy, igy, pary);
                if (fminf(tnx, tny) > fminf(te, b.t)) break;
                if (tnx <= tny) bx += sx; else by += sy;
                if (bx < 0 || by < 0 || bx >= p.c2x || by >= p.c2y) break;
            }
        }
    }

    // ---- shading
    float alb[3], rgb[3];
    if (b.id == RR_ID_SKY) {
        sky_colour(d, rgb);
    } else {
        if (b.id == RR_ID_GROUND) {
            // the hit triangle of cell (ix, iy): lower (fx >= fy) corners 00, 01, 11; upper 00, 10, 11
            const size_t c0 = (size_t)mh.iy * p.W + mh.ix;
            const float *q = p.height + c0;
            const float h00 = q[0], h01 = q[1], h10 = q[p.W], h11 = q[p.W + 1];
            const float a = mh.lower ? h01 - h00 : h11 - h10, bb = mh.lower ? h11 - h01 : h10 - h00;
            b.n[0] = -a * p.inv_res; b.n[1] = -bb * p.inv_res; b.n[2] = 1.0f;
            const float nn = 1.0f / sqrtf(dot3(b.n, b.n));
            const float s = dot3(b.n, d) > 0.0f ? -nn : nn;
            for (int i = 0; i < 3; ++i) b.n[i] *= s;
            if (p.obstacle) {
                const float *ob = p.obstacle + c0;
                const float om = fmaxf(fmaxf(ob[0], ob[p.W + 1]), mh.lower ? ob[1] : ob[p.W]);
                if (om > RR_ROCK_EPS) b.id = RR_ID_ROCK;
            }
        }
        const int kind = b.id < RR_ID_ENV0 ? b.id : (b.id - RR_ID_ENV0) % RR_IDS_PER_ENV;
        const float g[3] = RR_ALBEDO_GROUND, r[3] = RR_ALBEDO_ROCK, ch[3] = RR_ALBEDO_CHASSIS, wh[3] = RR_ALBEDO_WHEEL,
                    tg[3] = RR_ALBEDO_TARGET;
        for (int i = 0; i < 3; ++i)
            alb[i] = b.id == RR_ID_GROUND ? g[i] : b.id == RR_ID_ROCK ? r[i] : kind == 0 ? ch[i] : kind == 7 ? tg[i] : wh[i];
        const float lp[3] = RR_LIGHT_POS;
        float l[3];
        for (int i = 0; i < 3; ++i) l[i] = lp[i] - (o[i] + b.t * d[i]);
        const float ln = 1.0f / sqrtf(dot3(l, l));
        const float shade = RR_K_AMBIENT + RR_K_DIFFUSE * fmaxf(dot3(b.n, l) * ln, 0.0f);
        for (int i = 0; i < 3; ++i) rgb[i] = alb[i] * shade;
    }
    const size_t px = (size_t)v * p.cam.img_w + u;
    p.rgba[px] = pack_rgba(rgb);
    if (p.depth) p.depth[px] = b.id == RR_ID_SKY ? INFINITY : b.t;
    if (p.object_id) p.object_id[px] = b.id;
}

}  // namespace

extern "C" {

int rover_viewer_default_config(rover_viewer_config *c)
{
    if (!c) return rover_internal_fail(ROVER_ERR_INVALID, "cfg is NULL");
    default_view(c, 7.5f, 7.5f, 7.5f);                         // ORBIT ViewerCfg
    return ROVER_OK;
}

size_t rover_viewer_config_bytes(void) { return sizeof(rover_viewer_config); }

size_t rover_viewer_workspace_bytes(const rover_sim *sim, const rover_viewer_config *cfg)
{
    if (!sim) return 0;
    const rover_sim_view s = rover_internal_view(const_cast<rover_sim *>(sim));
    if (!s.have_terrain || !view_config_ok(cfg, s.n)) return 0;
    return layout_of(s).bytes;
}

int rover_viewer_prepare(rover_sim *sim, const rover_viewer_config *cfg, void *ws, size_t bytes, void *stream)
{
    if (!sim || !ws) return rover_internal_fail(ROVER_ERR_INVALID, "sim / ws is NULL");
    const rover_sim_view s = rover_internal_view(sim);
    if (!view_config_ok(cfg, s.n)) return rover_internal_fail(ROVER_ERR_INVALID, "invalid rover_viewer_config");
    if (!s.have_terrain) return rover_internal_fail(ROVER_ERR_STATE, "rover_set_terrain has not been called");
    DeviceGuard guard(s.device);
    if (bytes < layout_of(s).bytes) return rover_internal_fail(ROVER_ERR_INVALID, "viewer workspace too small");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return rover_internal_fail(ROVER_ERR_INVALID, "viewer workspace must be 256-byte aligned");
    const int rc = rover_internal_build_pyramid(s, ws, stream);
    if (rc != ROVER_OK) return rc;
    *s.viewer_ws = ws;
    *s.viewer_gen = s.terrain_gen;
    return ROVER_OK;
}

int rover_viewer_render(rover_sim *sim, const rover_viewer_config *cfg, void *ws, uint32_t *rgba, float *depth, int32_t *object_id,
                        void *stream)
{
    if (!sim || !ws || !rgba) return rover_internal_fail(ROVER_ERR_INVALID, "sim / ws / rgba is NULL");
    const rover_sim_view s = rover_internal_view(sim);
    if (!view_config_ok(cfg, s.n)) return rover_internal_fail(ROVER_ERR_INVALID, "invalid rover_viewer_config");
    if (!s.have_terrain) return rover_internal_fail(ROVER_ERR_STATE, "rover_set_terrain has not been called");
    if (!s.state) return rover_internal_fail(ROVER_ERR_STATE, "rover_bind has not been called");
    if (s.phase_open) return rover_internal_fail(ROVER_ERR_STATE, "rover_viewer_render between rover_step_begin and rover_step_finish");
    if (*s.viewer_ws != ws || *s.viewer_gen != s.terrain_gen)
        return rover_internal_fail(ROVER_ERR_STATE, "viewer workspace not prepared for the terrain bound now (call rover_viewer_prepare)");
    DeviceGuard guard(s.device);
    const Layout L = layout_of(s);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *base = static_cast<char *>(ws);

    BinParams bp;
    bp.state = s.state; bp.n = s.n; bp.W = s.W; bp.H = s.H; bp.c2x = L.py.c2x; bp.c2y = L.py.c2y;
    bp.inv_res = 1.0f / s.res; bp.min_x = s.min_x; bp.min_y = s.min_y;
    bp.rover_r = L.rover_r; bp.draw_targets = cfg->draw_targets != 0;
    bp.counts = reinterpret_cast<int *>(base + L.off_cnt);
    bp.start = reinterpret_cast<int *>(base + L.off_start);
    bp.cursor = reinterpret_cast<int *>(base + L.off_cur);
    bp.items = reinterpret_cast<int *>(base + L.off_items);
    bp.ovf = reinterpret_cast<int *>(base + L.off_ovf);
    bp.pose = reinterpret_cast<float *>(base + L.off_pose);
    const unsigned item_blocks = (unsigned)((L.n_items + 255) / 256);
    HIP_TRY(hipMemsetAsync(bp.counts, 0, (size_t)(L.nb + 1) * sizeof(int), st));
    if (item_blocks) hipLaunchKernelGGL(viewer_bin_count_kernel, dim3(item_blocks), dim3(256), 0, st, bp);
    hipLaunchKernelGGL(viewer_bin_scan_kernel, dim3(1), dim3(256), 0, st, bp);
    if (item_blocks) hipLaunchKernelGGL(viewer_bin_scatter_kernel, dim3(item_blocks), dim3(256), 0, st, bp);

    ViewParams p;
    p.height = s.height; p.obstacle = s.obstacle;
    p.l1 = reinterpret_cast<const float *>(base + L.py.off1);
    p.l2 = reinterpret_cast<const float *>(base + L.py.off2);
    p.zmax = reinterpret_cast<const float *>(base + L.py.offz);
    p.H = s.H; p.W = s.W; p.c1x = L.py.c1x; p.c2x = L.py.c2x; p.c2y = L.py.c2y;
    p.inv_res = 1.0f / s.res; p.min_x = s.min_x; p.min_y = s.min_y;
    p.state = s.state; p.n = s.n;
    p.origin_env = cfg->origin_type == ROVER_VIEWER_ORIGIN_ENV ? cfg->env_index : -1;
    p.draw_targets = bp.draw_targets;
    p.start = bp.start; p.items = bp.items; p.ovf_count = bp.counts + L.nb; p.ovf = bp.ovf; p.pose = bp.pose;
    p.rover_r = L.rover_r;
    p.cam = pinhole_of(cfg, nullptr);                              // ENV origin: the kernel adds the env's ROVER_POS
    p.near_clip = cfg->near_clip; p.far_clip = cfg->far_clip;
    p.rgba = rgba; p.depth = depth; p.object_id = object_id;
    const unsigned blocks = (unsigned)((p.cam.tiles + WAVES - 1) / WAVES);
    hipLaunchKernelGGL(rover_viewer_render_kernel, dim3(blocks), dim3(TILE * TILE * WAVES), 0, st, p);
    HIP_TRY(hipGetLastError());
    return ROVER_OK;
}

}  // extern "C"
