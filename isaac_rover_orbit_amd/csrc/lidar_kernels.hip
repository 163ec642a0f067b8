// lidar_kernels.hip -- the rover's scanning lidar (gfx950 / CDNA4, wave64): a caller-supplied table of Body-frame rays cast from each
// env's pose against the terrain's triangle mesh.
//
// See include/rover_lidar.h for the contract and the operation order.  The march is the depth camera's (terrain_march.hpp) and so is
// the workspace (the max-height pyramid, rover_internal_build_pyramid); what is new is the mapping.  One wave takes 64 CONSECUTIVE
// table entries of one env, so the env index -- and with it the pose, both frames and the origin -- is wave-uniform (scalar loads of
// the SoA state words), and which rays march together is decided by the order of the caller's table: lidar.pattern_rays emits it
// channel-major, so a wave holds one ring of equal elevation angle, where the camera's 8 x 8 tile mixes eight.  4 waves per
// workgroup; a tail wave masks the lanes past the table's end.  No LDS, no scratch; outputs leave with nontemporal stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/rover_hip.h"
#include "../../include/rover_lidar.h"
#include "rover_internal.hpp"
#include "terrain_march.hpp"

namespace {

using terrain_march::Pyramid;
using terrain_march::pyramid_of;

constexpr int WAVES = 4;     // waves per workgroup

struct LidarParams {
    const float *state;
    const float *height;
    const float *l1, *l2, *zmax;
    const float *ray_b;
    float *range, *hits;
    long long pitch;
    int n, H, W;
    int c1x, c2x;
    float inv_res, min_x, min_y;
    int rays, waves_per_env, yaw_only;
    float tm[3];
    float near_clip, far_clip;
};

// One wave per 64 consecutive table entries of one env.  The march's loops are per lane; a lane leaves them at its ray's hit or miss.
__global__ __launch_bounds__(64 * WAVES) void rover_lidar_cast_kernel(LidarParams p)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    const int env = __builtin_amdgcn_readfirstlane(wave / p.waves_per_env);
    if (env >= p.n) return;
    const int k = (wave - env * p.waves_per_env) * 64 + (threadIdx.x & 63);
    if (k >= p.rays) return;

    // ---- pose of the env (wave-uniform: scalar loads of the state words), header steps 1 - 3
    const float *S = p.state;
    const size_t N = (size_t)p.n;
    const float px = S[ROVER_POS * N + env], py = S[(ROVER_POS + 1) * N + env], pz = S[(ROVER_POS + 2) * N + env];
    float qw = S[ROVER_QUAT * N + env], qx = S[(ROVER_QUAT + 1) * N + env];
    float qy = S[(ROVER_QUAT + 2) * N + env], qz = S[(ROVER_QUAT + 3) * N + env];
    const float qn = 1.0f / sqrtf(__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(qw, qw), __fmul_rn(qx, qx)), __fmul_rn(qy, qy)), __fmul_rn(qz, qz)));
    qw = __fmul_rn(qw, qn); qx = __fmul_rn(qx, qn); qy = __fmul_rn(qy, qn); qz = __fmul_rn(qz, qn);
    const float xx = __fmul_rn(qx, qx), yy = __fmul_rn(qy, qy), zz = __fmul_rn(qz, qz);
    const float xy = __fmul_rn(qx, qy), xz = __fmul_rn(qx, qz), yz = __fmul_rn(qy, qz);
    const float wx = __fmul_rn(qw, qx), wy = __fmul_rn(qw, qy), wz = __fmul_rn(qw, qz);
    float R[9];
    R[0] = __fsub_rn(1.0f, __fmul_rn(2.0f, __fadd_rn(yy, zz)));
    if (p.yaw_only) {                                                // kernel argument: uniform
        const float a = R[0], b = __fmul_rn(2.0f, __fadd_rn(wz, xy));
        const float i2 = 1.0f / sqrtf(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)));
        const float cyaw = __fmul_rn(a, i2), syaw = __fmul_rn(b, i2);
        R[0] = cyaw; R[1] = -syaw; R[2] = 0.0f;
        R[3] = syaw; R[4] = cyaw; R[5] = 0.0f;
        R[6] = 0.0f; R[7] = 0.0f; R[8] = 1.0f;
    } else {
        R[1] = __fmul_rn(2.0f, __fsub_rn(xy, wz)); R[2] = __fmul_rn(2.0f, __fadd_rn(xz, wy));
        R[3] = __fmul_rn(2.0f, __fadd_rn(xy, wz)); R[4] = __fsub_rn(1.0f, __fmul_rn(2.0f, __fadd_rn(xx, zz)));
        R[5] = __fmul_rn(2.0f, __fsub_rn(yz, wx));
        R[6] = __fmul_rn(2.0f, __fsub_rn(xz, wy)); R[7] = __fmul_rn(2.0f, __fadd_rn(yz, wx));
        R[8] = __fsub_rn(1.0f, __fmul_rn(2.0f, __fadd_rn(xx, yy)));
    }
    auto row = [&](int i, float x, float y, float z) {
        return __fadd_rn(__fadd_rn(__fmul_rn(R[3 * i], x), __fmul_rn(R[3 * i + 1], y)), __fmul_rn(R[3 * i + 2], z));
    };
    const float ox = __fadd_rn(px, row(0, p.tm[0], p.tm[1], p.tm[2]));
    const float oy = __fadd_rn(py, row(1, p.tm[0], p.tm[1], p.tm[2]));
    const float oz = __fadd_rn(pz, row(2, p.tm[0], p.tm[1], p.tm[2]));

    // ---- the lane's ray: table entry k, step 4
    const float *r = p.ray_b + 3 * (size_t)k;                        // k < rays
    const float rx = r[0], ry = r[1], rz = r[2];
    const float dx = row(0, rx, ry, rz), dy = row(1, rx, ry, rz), dz = row(2, rx, ry, rz);

    terrain_march::MarchHit hit;
    const float t = terrain_march::march_terrain<false>(p, ox, oy, oz, dx, dy, dz, hit);
    __builtin_nontemporal_store(t, p.range + ((size_t)env * (size_t)p.pitch + (size_t)k));   // 64-bit; k < rays <= pitch
    if (p.hits) {                                                    // kernel argument: uniform
        const bool miss = !(t < INFINITY);
        float *h = p.hits + ((size_t)env * (size_t)p.rays + (size_t)k) * 3;
        __builtin_nontemporal_store(miss ? INFINITY : __fadd_rn(ox, __fmul_rn(t, dx)), h);
        __builtin_nontemporal_store(miss ? INFINITY : __fadd_rn(oy, __fmul_rn(t, dy)), h + 1);
        __builtin_nontemporal_store(miss ? INFINITY : __fadd_rn(oz, __fmul_rn(t, dz)), h + 2);
    }
}

// what the arguments alone decide (rover_lidar.h): the text of the refusal, or NULL
const char *refusal(const rover_sim *sim, const rover_lidar_config *c, const void *ws, const float *ray_b, const float *range,
                    int64_t pitch_floats, const float *hits_w)
{
    if (!sim || !c || !ws || !ray_b || !range) return "NULL argument (sim, cfg, ws, ray_b and range are required)";
    if (c->rays <= 0) return "rays must be >= 1";
    if (pitch_floats < (int64_t)c->rays) return "pitch_floats must be >= rays";
    if (pitch_floats > ((int64_t)1 << 29)) return "pitch_floats must be <= 2^29";
    if ((reinterpret_cast<uintptr_t>(ray_b) | reinterpret_cast<uintptr_t>(range) | reinterpret_cast<uintptr_t>(hits_w)) & 3)
        return "float pointers must be 4-byte aligned";
    if (!(std::isfinite(c->mount_pos[0]) && std::isfinite(c->mount_pos[1]) && std::isfinite(c->mount_pos[2])))
        return "mount_pos must be finite";
    if (!(c->near_clip >= 0.0f && c->near_clip < c->far_clip)) return "the clips must satisfy 0 <= near_clip < far_clip";
    if (c->attach_yaw_only != 0 && c->attach_yaw_only != 1) return "attach_yaw_only must be 0 or 1";
    return nullptr;
}

}  // namespace

extern "C" {

size_t rover_lidar_config_bytes(void) { return sizeof(rover_lidar_config); }

size_t rover_lidar_workspace_bytes(const rover_sim *sim)
{
    if (!sim) return 0;
    const rover_sim_view s = rover_internal_view(const_cast<rover_sim *>(sim));
    if (!s.have_terrain) return 0;
    return pyramid_of(s.H, s.W).bytes;
}

int rover_lidar_prepare(rover_sim *sim, void *ws, size_t bytes, void *stream)
{
    if (!sim || !ws) return rover_internal_fail(ROVER_ERR_INVALID, "rover_lidar_prepare: %s", "sim / ws is NULL");
    if (reinterpret_cast<uintptr_t>(ws) & 255)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_lidar_prepare: %s", "the workspace must be 256-byte aligned");
    const rover_sim_view s = rover_internal_view(sim);
    if (!s.have_terrain) return rover_internal_fail(ROVER_ERR_STATE, "rover_lidar_prepare: %s", "rover_set_terrain has not been called");
    if (bytes < pyramid_of(s.H, s.W).bytes) return rover_internal_fail(ROVER_ERR_INVALID, "rover_lidar_prepare: %s", "workspace too small");
    DeviceGuard guard(s.device);
    const int rc = rover_internal_build_pyramid(s, ws, stream);
    if (rc != ROVER_OK) return rc;
    *s.camera_ws = ws;                                               // the camera's record: one workspace serves both sensors
    *s.camera_gen = s.terrain_gen;
    return ROVER_OK;
}

int rover_lidar_cast(rover_sim *sim, const rover_lidar_config *cfg, const void *ws, const float *ray_b, float *range,
                     int64_t pitch_floats, float *hits_w, void *stream)
{
    static const char who[] = "rover_lidar_cast: %s";
    if (const char *why = refusal(sim, cfg, ws, ray_b, range, pitch_floats, hits_w)) return rover_internal_fail(ROVER_ERR_INVALID, who, why);
    const rover_sim_view s = rover_internal_view(sim);
    if (!s.have_terrain) return rover_internal_fail(ROVER_ERR_STATE, who, "rover_set_terrain has not been called");
    if (!s.state) return rover_internal_fail(ROVER_ERR_STATE, who, "rover_bind has not been called");
    if (s.phase_open) return rover_internal_fail(ROVER_ERR_STATE, who, "called between rover_step_begin and rover_step_finish");
    if (*s.camera_ws != ws || *s.camera_gen != s.terrain_gen)
        return rover_internal_fail(ROVER_ERR_STATE, who, "workspace not prepared for the terrain bound now (call rover_lidar_prepare)");
    const int wpe = (int)(((int64_t)cfg->rays + 63) / 64);
    const uint64_t blocks = ((uint64_t)s.n * (uint64_t)wpe + WAVES - 1) / WAVES;
    if (blocks > 0x7FFFFFFFull) return rover_internal_fail(ROVER_ERR_UNSUPPORTED, who, "too many rays for one launch");
    DeviceGuard guard(s.device);
    const Pyramid py = pyramid_of(s.H, s.W);
    const char *base = static_cast<const char *>(ws);
    LidarParams p;
    p.state = s.state; p.height = s.height;
    p.l1 = reinterpret_cast<const float *>(base + py.off1);
    p.l2 = reinterpret_cast<const float *>(base + py.off2);
    p.zmax = reinterpret_cast<const float *>(base + py.offz);
    p.ray_b = ray_b; p.range = range; p.hits = hits_w;
    p.pitch = (long long)pitch_floats;
    p.n = s.n; p.H = s.H; p.W = s.W; p.c1x = py.c1x; p.c2x = py.c2x;
    p.inv_res = 1.0f / s.res; p.min_x = s.min_x; p.min_y = s.min_y;
    p.rays = cfg->rays; p.waves_per_env = wpe; p.yaw_only = cfg->attach_yaw_only;
    for (int i = 0; i < 3; ++i) p.tm[i] = cfg->mount_pos[i];
    p.near_clip = cfg->near_clip; p.far_clip = cfg->far_clip;
    hipLaunchKernelGGL(rover_lidar_cast_kernel, dim3((unsigned)blocks), dim3(64 * WAVES), 0, static_cast<hipStream_t>(stream), p);
    return launched("rover_lidar_cast_kernel launch: %s");
}

}  // extern "C"
