// camera_kernels.hip -- the rover's on-board depth camera (gfx950): a ray march over the terrain's triangle mesh.
//
// Reference: rover_envs/envs/navigation/entrypoints/rover_camera_env.py:18-104 (RoverEnvCamera, the `distance_to_camera`
// annotator of one render product per env).  The scene's only geometry is the terrain mesh, i.e. the heightfield bound to the
// rover_sim handle with every cell split along its (i, j) - (i+1, j+1) diagonal -- the surface the height scanner casts against.
//
// prepare: a max-height pyramid over the heightfield (8 x 8 and 64 x 64 cells per block, plus the global maximum).
// render:  one wave = one 8 x 8 pixel tile of one env; each lane marches its pixel's ray (terrain_march.hpp) with a 2-D DDA over the cells,
//          skipping a 64 x 64 or 8 x 8 block whenever the ray stays above the block's maximum over the block's whole t-range.
//          Inside a cell the ray is split at the cell's diagonal and tested against the plane of each triangle it passes.
//          The signed vertical gap ray - surface is continuous along the ray (the mesh is), so it is carried from one cell
//          boundary to the next: two plane evaluations per cell, and a crossing on a cell boundary cannot slip between cells.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/rover_camera.h"
#include "../../include/rover_hip.h"
#include "rover_internal.hpp"
#include "terrain_march.hpp"

namespace {

using terrain_march::L1;
using terrain_march::L2;
using terrain_march::Pyramid;
using terrain_march::pyramid_of;

constexpr int TILE = 8;      // pixels per side of a wave's tile
constexpr int WAVES = 4;     // waves (tiles) per workgroup

// block (bx, by) of `level` cells per side: max over the heightfield NODES of its cells, nodes [level * b, level * b + level]
__global__ void camera_block_max_kernel(const float *__restrict__ height, int H, int W, int level, int cx, int cy,
                                        float *__restrict__ out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= cx * cy) return;
    const int bx = b % cx, by = b / cx;
    const int i0 = by * level, i1 = min(i0 + level, H - 1);
    const int j0 = bx * level, j1 = min(j0 + level, W - 1);
    float m = -INFINITY;
    for (int i = i0; i <= i1; ++i)
        for (int j = j0; j <= j1; ++j) m = fmaxf(m, height[(size_t)i * W + j]);
    out[b] = m;
}

__global__ void camera_global_max_kernel(const float *__restrict__ l2, int n, float *__restrict__ zmax)
{
    __shared__ float red[256];
    float m = -INFINITY;
    for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, l2[i]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *zmax = red[0];
}

struct CamParams {
    const float *state;
    const float *height;
    const float *l1, *l2, *zmax;
    float *depth;
    int n, H, W;
    int c1x, c2x;
    float inv_res, min_x, min_y;
    int img_w, img_h, tiles_x, tiles_per_env;
    float inv_fx, inv_fy, half_w, half_h;
    float Rm[9];             // Body <- camera rotation of the (normalised) mount quaternion
    float tm[3];             // mount translation in the Body frame
    float near_clip, far_clip;
};

// One wave per 8 x 8 tile of one env.  Every loop below is per lane; a lane leaves it at its ray's hit or miss.
__global__ __launch_bounds__(TILE * TILE * WAVES) void rover_camera_render_kernel(CamParams p)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    const int env = __builtin_amdgcn_readfirstlane(wave / p.tiles_per_env);
    if (env >= p.n) return;
    const int tile = wave - env * p.tiles_per_env;
    const int lane = threadIdx.x & 63;
    const int u = (tile % p.tiles_x) * TILE + (lane & (TILE - 1));
    const int v = (tile / p.tiles_x) * TILE + (lane >> 3);
    if (u >= p.img_w || v >= p.img_h) return;

    // ---- camera pose of the env (wave-uniform: scalar loads of the state words)
    const float *S = p.state;
    const size_t N = (size_t)p.n;
    const float px = S[ROVER_POS * N + env], py = S[(ROVER_POS + 1) * N + env], pz = S[(ROVER_POS + 2) * N + env];
    float qw = S[ROVER_QUAT * N + env], qx = S[(ROVER_QUAT + 1) * N + env];
    float qy = S[(ROVER_QUAT + 2) * N + env], qz = S[(ROVER_QUAT + 3) * N + env];
    const float qn = 1.0f / sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
    qw *= qn; qx *= qn; qy *= qn; qz *= qn;
    float Rb[9];
    Rb[0] = 1.0f - 2.0f * (qy * qy + qz * qz); Rb[1] = 2.0f * (qx * qy - qw * qz); Rb[2] = 2.0f * (qx * qz + qw * qy);
    Rb[3] = 2.0f * (qx * qy + qw * qz); Rb[4] = 1.0f - 2.0f * (qx * qx + qz * qz); Rb[5] = 2.0f * (qy * qz - qw * qx);
    Rb[6] = 2.0f * (qx * qz - qw * qy); Rb[7] = 2.0f * (qy * qz + qw * qx); Rb[8] = 1.0f - 2.0f * (qx * qx + qy * qy);
    const float ox = px + Rb[0] * p.tm[0] + Rb[1] * p.tm[1] + Rb[2] * p.tm[2];
    const float oy = py + Rb[3] * p.tm[0] + Rb[4] * p.tm[1] + Rb[5] * p.tm[2];
    const float oz = pz + Rb[6] * p.tm[0] + Rb[7] * p.tm[1] + Rb[8] * p.tm[2];

    // ---- ray of pixel (u, v) through its centre: camera frame (x right, y up, looking along -z), then Body, then world
    const float cxr = ((float)u + 0.5f - p.half_w) * p.inv_fx;
    const float cyr = -((float)v + 0.5f - p.half_h) * p.inv_fy;
    const float cn = 1.0f / sqrtf(cxr * cxr + cyr * cyr + 1.0f);
    const float c0 = cxr * cn, c1 = cyr * cn, c2 = -cn;
    const float bx = p.Rm[0] * c0 + p.Rm[1] * c1 + p.Rm[2] * c2;
    const float by = p.Rm[3] * c0 + p.Rm[4] * c1 + p.Rm[5] * c2;
    const float bz = p.Rm[6] * c0 + p.Rm[7] * c1 + p.Rm[8] * c2;
    const float dx = Rb[0] * bx + Rb[1] * by + Rb[2] * bz;
    const float dy = Rb[3] * bx + Rb[4] * by + Rb[5] * bz;
    const float dz = Rb[6] * bx + Rb[7] * by + Rb[8] * bz;

    terrain_march::MarchHit hit;
    const float depth = terrain_march::march_terrain<false>(p, ox, oy, oz, dx, dy, dz, hit);
    const size_t o = ((size_t)env * p.img_h + v) * p.img_w + u;   // 64-bit: N x 14 400 passes 2^31 at 149 k envs
    __builtin_nontemporal_store(depth, p.depth + o);
}

// far_clip may be +inf; every other float is finite (a non-finite lens or mount would give all-miss or degenerate images)
bool config_ok(const rover_camera_config *c)
{
    if (!c) return false;
    for (float v : {c->focal_length, c->horizontal_aperture, c->vertical_aperture, c->mount_pos[0], c->mount_pos[1], c->mount_pos[2],
                    c->mount_quat[0], c->mount_quat[1], c->mount_quat[2], c->mount_quat[3]})
        if (!std::isfinite(v)) return false;
    return c->width > 0 && c->height > 0 && c->focal_length > 0.0f && c->horizontal_aperture > 0.0f && c->near_clip >= 0.0f &&
           c->near_clip < c->far_clip &&
           (c->mount_quat[0] != 0.0f || c->mount_quat[1] != 0.0f || c->mount_quat[2] != 0.0f || c->mount_quat[3] != 0.0f);
}

}  // namespace

// the max-height pyramid of the terrain bound to `s` into ws[0, pyramid_of(H, W).bytes) (camera and viewer workspaces alike)
int rover_internal_build_pyramid(const rover_sim_view &s, void *ws, void *stream)
{
    const Pyramid py = pyramid_of(s.H, s.W);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *base = static_cast<char *>(ws);
    float *l1 = reinterpret_cast<float *>(base + py.off1), *l2 = reinterpret_cast<float *>(base + py.off2);
    float *zmax = reinterpret_cast<float *>(base + py.offz);
    const int n1 = py.c1x * py.c1y, n2 = py.c2x * py.c2y;
    hipLaunchKernelGGL(camera_block_max_kernel, dim3((n1 + 255) / 256), dim3(256), 0, st, s.height, s.H, s.W, L1, py.c1x, py.c1y, l1);
    hipLaunchKernelGGL(camera_block_max_kernel, dim3((n2 + 255) / 256), dim3(256), 0, st, s.height, s.H, s.W, L2, py.c2x, py.c2y, l2);
    hipLaunchKernelGGL(camera_global_max_kernel, dim3(1), dim3(256), 0, st, l2, n2, zmax);
    HIP_TRY(hipGetLastError());
    return ROVER_OK;
}

extern "C" {

int rover_camera_default_config(rover_camera_config *c)
{
    if (!c) return rover_internal_fail(ROVER_ERR_INVALID, "cfg is NULL");
    c->width = 160; c->height = 90;                        // rover_camera_env.py:62 render product
    c->focal_length = 2.12f;                               // :47
    c->horizontal_aperture = 6.055f;                       // :49
    c->vertical_aperture = 0.0f;                           // square pixels (Isaac Sim derives it from the aspect ratio); :50 states 2.968879962
    c->mount_pos[0] = -0.151f; c->mount_pos[1] = 0.0f; c->mount_pos[2] = 0.73428f;                          // :55
    c->mount_quat[0] = 0.64086f; c->mount_quat[1] = 0.29884f; c->mount_quat[2] = -0.29884f; c->mount_quat[3] = -0.64086f;  // :56
    c->near_clip = 0.01f; c->far_clip = 1000000.0f;        // :51
    return ROVER_OK;
}

size_t rover_camera_config_bytes(void) { return sizeof(rover_camera_config); }

size_t rover_camera_workspace_bytes(const rover_sim *sim, const rover_camera_config *cfg)
{
    if (!sim || !config_ok(cfg)) return 0;
    const rover_sim_view s = rover_internal_view(const_cast<rover_sim *>(sim));
    if (!s.have_terrain) return 0;
    return pyramid_of(s.H, s.W).bytes;
}

int rover_camera_prepare(rover_sim *sim, const rover_camera_config *cfg, void *ws, size_t bytes, void *stream)
{
    if (!sim || !ws) return rover_internal_fail(ROVER_ERR_INVALID, "sim / ws is NULL");
    if (!config_ok(cfg)) return rover_internal_fail(ROVER_ERR_INVALID, "invalid rover_camera_config");
    const rover_sim_view s = rover_internal_view(sim);
    if (!s.have_terrain) return rover_internal_fail(ROVER_ERR_STATE, "rover_set_terrain has not been called");
    DeviceGuard guard(s.device);
    const Pyramid py = pyramid_of(s.H, s.W);
    if (bytes < py.bytes) return rover_internal_fail(ROVER_ERR_INVALID, "camera workspace too small");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return rover_internal_fail(ROVER_ERR_INVALID, "camera workspace must be 256-byte aligned");
    const int rc = rover_internal_build_pyramid(s, ws, stream);
    if (rc != ROVER_OK) return rc;
    *s.camera_ws = ws;
    *s.camera_gen = s.terrain_gen;
    return ROVER_OK;
}

int rover_camera_render(rover_sim *sim, const rover_camera_config *cfg, const void *ws, float *depth, void *stream)
{
    if (!sim || !ws || !depth) return rover_internal_fail(ROVER_ERR_INVALID, "sim / ws / depth is NULL");
    if (!config_ok(cfg)) return rover_internal_fail(ROVER_ERR_INVALID, "invalid rover_camera_config");
    const rover_sim_view s = rover_internal_view(sim);
    if (!s.have_terrain) return rover_internal_fail(ROVER_ERR_STATE, "rover_set_terrain has not been called");
    if (!s.state) return rover_internal_fail(ROVER_ERR_STATE, "rover_bind has not been called");
    if (s.phase_open) return rover_internal_fail(ROVER_ERR_STATE, "rover_camera_render between rover_step_begin and rover_step_finish");
    if (*s.camera_ws != ws || *s.camera_gen != s.terrain_gen)
        return rover_internal_fail(ROVER_ERR_STATE, "camera workspace not prepared for the terrain bound now (call rover_camera_prepare)");
    DeviceGuard guard(s.device);
    const Pyramid py = pyramid_of(s.H, s.W);
    const char *base = static_cast<const char *>(ws);
    CamParams p;
    p.state = s.state; p.height = s.height;
    p.l1 = reinterpret_cast<const float *>(base + py.off1);
    p.l2 = reinterpret_cast<const float *>(base + py.off2);
    p.zmax = reinterpret_cast<const float *>(base + py.offz);
    p.depth = depth;
    p.n = s.n; p.H = s.H; p.W = s.W; p.c1x = py.c1x; p.c2x = py.c2x;
    p.inv_res = 1.0f / s.res; p.min_x = s.min_x; p.min_y = s.min_y;
    p.img_w = cfg->width; p.img_h = cfg->height;
    p.tiles_x = (cfg->width + TILE - 1) / TILE;
    p.tiles_per_env = p.tiles_x * ((cfg->height + TILE - 1) / TILE);
    const double fx = (double)cfg->width * cfg->focal_length / cfg->horizontal_aperture;
    const double fy = cfg->vertical_aperture > 0.0f ? (double)cfg->height * cfg->focal_length / cfg->vertical_aperture : fx;
    p.inv_fx = (float)(1.0 / fx); p.inv_fy = (float)(1.0 / fy);
    p.half_w = 0.5f * (float)cfg->width; p.half_h = 0.5f * (float)cfg->height;
    double q[4] = {cfg->mount_quat[0], cfg->mount_quat[1], cfg->mount_quat[2], cfg->mount_quat[3]};
    const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (double &x : q) x /= qn;
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 9; ++i) p.Rm[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) p.tm[i] = cfg->mount_pos[i];
    p.near_clip = cfg->near_clip; p.far_clip = cfg->far_clip;
    const uint64_t waves = (uint64_t)s.n * (uint64_t)p.tiles_per_env;
    const uint64_t blocks = (waves + WAVES - 1) / WAVES;
    if (blocks > 0x7FFFFFFFull) return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "too many pixels for one launch");
    hipLaunchKernelGGL(rover_camera_render_kernel, dim3((unsigned)blocks), dim3(TILE * TILE * WAVES), 0,
                       static_cast<hipStream_t>(stream), p);
    HIP_TRY(hipGetLastError());
    return ROVER_OK;
}

}  // extern "C"
