// viewer_common.hpp -- what the two rgb_array viewers (viewer_kernels.hip, lift_viewer_kernels.hip) share: the pinhole camera as a
// kernel argument, the hit rule, the marker sphere, the sky, the colour packing, and the host code that checks a config and builds
// the camera from it.  DESIGN.md section 37 is the image contract; it also says which of its lines each render kernel still
// carries itself (tile prologue, pixel ray, shade factor, depth / id stores) and why.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/rover_lift_viewer.h"
#include "rover_render.hpp"

namespace viewer_common {

constexpr int TILE = 8;         // pixels per side of a wave's tile
constexpr int WAVES = 4;        // waves (tiles) per workgroup

// The camera of a frame, as both ViewParams embed it (4-byte members only: it does not move the kernel arguments around it).
struct Pinhole {
    int img_w, img_h, tiles_x, tiles;
    float eye[3], fwd[3], right[3], up[3];
    float inv_f, half_w, half_h;
};

struct Best {
    float t;
    int id;
    float n[3];                  // geometric normal facing the ray (objects; the rover's terrain normal is formed at shading)
};

__device__ __forceinline__ float dot3(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// nearest hit wins, equal t goes to the lower id; `n` is the geometric normal of either sign and is stored facing the ray
__device__ __forceinline__ void offer(Best &b, float t, int id, const float *n, const float *d, float far_clip)
{
    if (t <= far_clip && (t < b.t || (t == b.t && id < b.id))) {
        const float s = dot3(n, d) > 0.0f ? -1.0f : 1.0f;
        b.t = t; b.id = id; b.n[0] = s * n[0]; b.n[1] = s * n[1]; b.n[2] = s * n[2];
    }
}

// [t0, t1] of the ray o + t d inside a sphere; false if it misses
__device__ __forceinline__ bool sphere_span(const float *o, const float *d, const float *c, float r, float &t0, float &t1)
{
    const float oc[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
    const float b = dot3(oc, d), cc = dot3(oc, oc) - r * r;
    const float disc = b * b - cc;
    if (!(disc >= 0.0f)) return false;
    const float sq = sqrtf(disc);
    t0 = -b - sq; t1 = -b + sq;
    return true;
}

// a marker sphere (the rover's target, the lift's goal): the first of its two crossings at or beyond near_clip
__device__ __forceinline__ void test_marker(const float *o, const float *d, const float *c, float r, float near_clip, float far_clip,
                                            int id, Best &b)
{
    float t0, t1;
    if (!sphere_span(o, d, c, r, t0, t1)) return;
    const float t = t0 >= near_clip ? t0 : t1;
    if (!(t >= near_clip)) return;
    float nrm[3];
    for (int i = 0; i < 3; ++i) nrm[i] = (o[i] + t * d[i] - c[i]) * (1.0f / r);
    offer(b, t, id, nrm, d, far_clip);
}

__device__ __forceinline__ void sky_colour(const float *d, float *rgb)
{
    const float hz[3] = RR_SKY_HORIZON, zn[3] = RR_SKY_ZENITH;
    const float w = fmaxf(d[2], 0.0f);
    for (int i = 0; i < 3; ++i) rgb[i] = hz[i] + (zn[i] - hz[i]) * w;
}

__device__ __forceinline__ uint32_t to_byte(float x) { return (uint32_t)rintf(255.0f * fminf(fmaxf(x, 0.0f), 1.0f)); }

// a colour as the rgba image stores it: a byte per channel, rounded to nearest, alpha 255
__device__ __forceinline__ uint32_t pack_rgba(const float *rgb)
{
    return to_byte(rgb[0]) | (to_byte(rgb[1]) << 8) | (to_byte(rgb[2]) << 16) | 0xFF000000u;
}

// ---- host side
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

inline double norm3(const double *v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// rover_lift_viewer_config begins with rover_viewer_config, member for member (lift_env.lift_viewer_native copies it by name)
#define VIEWER_SAME_MEMBER(m)                                                                                          \
    static_assert(offsetof(rover_lift_viewer_config, m) == offsetof(rover_viewer_config, m) &&                         \
                  sizeof(rover_lift_viewer_config::m) == sizeof(rover_viewer_config::m), "rover_lift_viewer_config: " #m " moved")
VIEWER_SAME_MEMBER(eye); VIEWER_SAME_MEMBER(lookat); VIEWER_SAME_MEMBER(origin_type); VIEWER_SAME_MEMBER(env_index);
VIEWER_SAME_MEMBER(width); VIEWER_SAME_MEMBER(height); VIEWER_SAME_MEMBER(focal_length); VIEWER_SAME_MEMBER(horizontal_aperture);
VIEWER_SAME_MEMBER(near_clip); VIEWER_SAME_MEMBER(far_clip); VIEWER_SAME_MEMBER(draw_targets);
#undef VIEWER_SAME_MEMBER
static_assert(offsetof(rover_lift_viewer_config, env_spacing) == sizeof(rover_viewer_config), "rover_lift_viewer_config: a member between");

// the checks both C entries make of the members above; `n` = the env count (env_index)
template <class Config>
bool view_config_ok(const Config *c, int n)
{
    if (!c) return false;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(c->eye[i]) || !std::isfinite(c->lookat[i])) return false;
    const double dx = (double)c->lookat[0] - c->eye[0], dy = (double)c->lookat[1] - c->eye[1];
    if (dx == 0.0 && dy == 0.0) return false;                      // eye == lookat, or a view along +-Z
    if (!(std::isfinite(c->focal_length) && std::isfinite(c->horizontal_aperture) && c->focal_length > 0.0f &&
          c->horizontal_aperture > 0.0f))
        return false;
    if (!(c->near_clip >= 0.0f && c->near_clip < c->far_clip)) return false;
    if (c->width < 1 || c->height < 1 || c->width > ROVER_VIEWER_MAX_SIZE || c->height > ROVER_VIEWER_MAX_SIZE) return false;
    if (c->origin_type == ROVER_VIEWER_ORIGIN_ENV) return c->env_index >= 0 && c->env_index < n;
    return c->origin_type == ROVER_VIEWER_ORIGIN_WORLD;
}

// the members above at their defaults: lookat (0, 0, 0), origin "world", 1280 x 720, Kit's default lens; the eye is the caller's
template <class Config>
void default_view(Config *c, float ex, float ey, float ez)
{
    c->eye[0] = ex; c->eye[1] = ey; c->eye[2] = ez;
    c->lookat[0] = c->lookat[1] = c->lookat[2] = 0.0f;
    c->origin_type = ROVER_VIEWER_ORIGIN_WORLD;
    c->env_index = 0;
    c->width = 1280; c->height = 720;
    c->focal_length = RR_FOCAL_LENGTH;
    c->horizontal_aperture = RR_HORIZONTAL_APERTURE;
    c->near_clip = RR_NEAR_CLIP; c->far_clip = RR_FAR_CLIP;
    c->draw_targets = 1;
}

// the camera of a valid config: forward = lookat - eye, right = forward x +Z, up = right x forward (float64, then rounded), the
// lens and the tiling.  `org` (may be NULL) is added to the eye in float64.
template <class Config>
Pinhole pinhole_of(const Config *cfg, const double *org)
{
    Pinhole c;
    c.img_w = cfg->width; c.img_h = cfg->height;
    c.tiles_x = (cfg->width + TILE - 1) / TILE;
    c.tiles = c.tiles_x * ((cfg->height + TILE - 1) / TILE);
    double f[3] = {(double)cfg->lookat[0] - cfg->eye[0], (double)cfg->lookat[1] - cfg->eye[1], (double)cfg->lookat[2] - cfg->eye[2]};
    const double fl = norm3(f);
    for (double &x : f) x /= fl;
    double r[3] = {f[1], -f[0], 0.0};
    const double rl = norm3(r);
    for (double &x : r) x /= rl;
    const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
    for (int i = 0; i < 3; ++i) {
        c.eye[i] = org ? (float)((double)cfg->eye[i] + org[i]) : cfg->eye[i];
        c.fwd[i] = (float)f[i]; c.right[i] = (float)r[i]; c.up[i] = (float)u[i];
    }
    c.inv_f = (float)((double)cfg->horizontal_aperture / ((double)cfg->width * cfg->focal_length));
    c.half_w = 0.5f * (float)cfg->width; c.half_h = 0.5f * (float)cfg->height;
    return c;
}

}  // namespace viewer_common
