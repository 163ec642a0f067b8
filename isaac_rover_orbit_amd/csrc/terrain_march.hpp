// terrain_march.hpp -- the ray march over the terrain's triangle mesh that the depth camera (camera_kernels.hip) and the viewer
// (viewer_kernels.hip) share: the max-height pyramid's layout, and the per-lane 2-D DDA with its block skip and cell test.
//
// The mesh is the heightfield bound to the rover_sim handle with every cell split along its (i, j) - (i+1, j+1) diagonal -- the
// surface the height scanner casts against.  The pyramid holds the maximum over 8 x 8 and 64 x 64 cell blocks plus the global
// maximum; camera_kernels.hip builds it (rover_internal_build_pyramid).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace terrain_march {

constexpr int L1 = 8;        // cells per side of a fine block
constexpr int L2 = 64;       // cells per side of a coarse block

struct Pyramid {
    int c1x, c1y, c2x, c2y;  // blocks per row / column of each level
    size_t off1, off2, offz, bytes;
};

inline Pyramid pyramid_of(int H, int W)
{
    Pyramid p;
    p.c1x = (W - 1 + L1 - 1) / L1; p.c1y = (H - 1 + L1 - 1) / L1;
    p.c2x = (W - 1 + L2 - 1) / L2; p.c2y = (H - 1 + L2 - 1) / L2;
    p.off1 = 0;
    p.off2 = (p.off1 + (size_t)p.c1x * p.c1y * sizeof(float) + 255) & ~(size_t)255;
    p.offz = (p.off2 + (size_t)p.c2x * p.c2y * sizeof(float) + 255) & ~(size_t)255;
    p.bytes = p.offz + 256;
    return p;
}

__device__ __forceinline__ float lo_boundary_t(float k, float g0, float inv_gd, bool par) { return par ? INFINITY : (k - g0) * inv_gd; }

// Where a march ended: the cell (ix, iy) of the hit and which of its two triangles (lower: fx >= fy, corners 00, 01, 11; upper:
// corners 00, 10, 11).  Written only when WANT_HIT and the returned depth is finite.
struct MarchHit {
    int ix, iy;
    bool lower;
};

// The first t in [p.near_clip, p.far_clip] at which the ray o + t d (d a unit vector) meets the mesh, +inf where there is none.
// `P` holds the terrain and the pyramid: height, l1, l2 (block maxima), zmax (-> the global maximum), H, W, c1x, c2x,
// inv_res, min_x, min_y, near_clip, far_clip.  Every loop is per lane; a lane leaves it at its ray's hit or miss.
//
// A block is skipped while the ray's lower end over the block's t-range is above the block's maximum.  Inside a cell the ray is
// split at the cell's diagonal and tested against the plane of each triangle it passes.  The signed vertical gap ray - surface is
// continuous along the ray (the mesh is), so it is carried from one cell boundary to the next: two plane evaluations per cell, and
// a crossing on a cell boundary cannot slip between cells.
template <bool WANT_HIT, class P>
__device__ __forceinline__ float march_terrain(const P &p, float ox, float oy, float oz, float dx, float dy, float dz, MarchHit &hit)
{
    // ---- grid coordinates (cells), the ray's t-range over the terrain's x-y extent and below its maximum
    const float gox = (ox - p.min_x) * p.inv_res, goy = (oy - p.min_y) * p.inv_res;
    const float gdx = dx * p.inv_res, gdy = dy * p.inv_res;
    const bool parx = gdx == 0.0f, pary = gdy == 0.0f;
    const float igx = parx ? 0.0f : 1.0f / gdx, igy = pary ? 0.0f : 1.0f / gdy;
    const float xmax = (float)(p.W - 1), ymax = (float)(p.H - 1);
    const float zmax = *p.zmax;
    float t_lo = p.near_clip, t_hi = p.far_clip;
    bool miss = !(isfinite(gox) && isfinite(goy) && isfinite(oz) && isfinite(gdx) && isfinite(gdy) && isfinite(dz));
    if (parx) miss |= !(gox >= 0.0f && gox <= xmax);
    else { const float a = -gox * igx, b = (xmax - gox) * igx; t_lo = fmaxf(t_lo, fminf(a, b)); t_hi = fminf(t_hi, fmaxf(a, b)); }
    if (pary) miss |= !(goy >= 0.0f && goy <= ymax);
    else { const float a = -goy * igy, b = (ymax - goy) * igy; t_lo = fmaxf(t_lo, fminf(a, b)); t_hi = fminf(t_hi, fmaxf(a, b)); }
    // a ray whose range starts where it descends through the terrain's maximum was above the surface before: it starts above
    // (decided here, not from the gap at t_lo, which rounding may put a hair below a surface that reaches the maximum there)
    bool from_top = false;
    if (dz > 0.0f) t_hi = fminf(t_hi, (zmax - oz) / dz);
    else if (dz < 0.0f) { const float tz = (zmax - oz) / dz; from_top = tz >= t_lo; t_lo = fmaxf(t_lo, tz); }
    else miss |= oz > zmax;
    miss |= !(t_lo <= t_hi);

    float depth = INFINITY;
    if (!miss) {
        const int sx = gdx > 0.0f ? 1 : -1, sy = gdy > 0.0f ? 1 : -1;
        const int ux = sx > 0, uy = sy > 0;           // next boundary of cell i in the direction of travel: i + ux
        int ix = min(max((int)floorf(fmaf(t_lo, gdx, gox)), 0), p.W - 2);
        int iy = min(max((int)floorf(fmaf(t_lo, gdy, goy)), 0), p.H - 2);
        float t = t_lo;
        float g = 0.0f;          // gap at t, valid when have_g
        bool have_g = false;
        int above = from_top ? 1 : -1;   // side of the surface the ray starts on (-1: not known yet; touching counts as above)
        bool check_blocks = true;
        const float *hf = p.height;
        const int W = p.W;
        for (;;) {
            if (check_blocks && above != 0) {
                // a block is skipped while the ray's lower end over the block's t-range is above the block's maximum
                bool skipped = false;
                for (int lv = 0; lv < 2 && !skipped; ++lv) {
                    const int B = lv == 0 ? L2 : L1;
                    const int bxi = ix / B, byi = iy / B;
                    const float bmax = lv == 0 ? p.l2[byi * p.c2x + bxi] : p.l1[byi * p.c1x + bxi];
                    const float tx = lo_boundary_t((float)((bxi + ux) * B), gox, igx, parx);
                    const float ty = lo_boundary_t((float)((byi + uy) * B), goy, igy, pary);
                    const float te = fminf(fminf(tx, ty), t_hi);
                    if (fminf(fmaf(t, dz, oz), fmaf(te, dz, oz)) > bmax) {
                        skipped = true;
                        above = 1;
                        have_g = false;
                        t = te;
                        if (te >= t_hi) break;
                        if (tx <= ty) {
                            ix = (bxi + ux) * B - (1 - ux);
                            const int jy = (int)floorf(fmaf(te, gdy, goy));
                            iy = sy > 0 ? min(max(jy, iy), byi * B + B - 1) : max(min(jy, iy), byi * B);
                        } else {
                            iy = (byi + uy) * B - (1 - uy);
                            const int jx = (int)floorf(fmaf(te, gdx, gox));
                            ix = sx > 0 ? min(max(jx, ix), bxi * B + B - 1) : max(min(jx, ix), bxi * B);
                        }
                    }
                }
                if (skipped) {
                    if (t >= t_hi || ix < 0 || iy < 0 || ix > p.W - 2 || iy > p.H - 2) break;
                    continue;
                }
                check_blocks = false;
            }
            // ---- cell (ix, iy) over [t, tc]
            const float tx = lo_boundary_t((float)(ix + ux), gox, igx, parx);
            const float ty = lo_boundary_t((float)(iy + uy), goy, igy, pary);
            const float tc = fmaxf(fminf(fminf(tx, ty), t_hi), t);
            const float *q = hf + (size_t)iy * W + ix;
            const float h00 = q[0], h01 = q[1], h10 = q[W], h11 = q[W + 1];
            const float fx0 = gox - (float)ix, fy0 = goy - (float)iy;
            // lower triangle (fx >= fy): corners 00, 01, 11; upper: 00, 10, 11
            auto gap = [&](float tt, bool lower) {
                const float a = lower ? h01 - h00 : h11 - h10, b = lower ? h11 - h01 : h10 - h00;
                const float fx = fmaf(tt, gdx, fx0), fy = fmaf(tt, gdy, fy0);
                return fmaf(tt, dz, oz) - fmaf(fy, b, fmaf(fx, a, h00));
            };
            // the diagonal fx = fy splits [t, tc] at tm
            const float e0 = fx0 - fy0, de = gdx - gdy;
            const float ea = fmaf(t, de, e0), eb = fmaf(tc, de, e0);
            float tm = tc;
            bool lowerA = ea + eb >= 0.0f;
            if ((ea >= 0.0f) != (eb >= 0.0f)) {
                tm = fminf(fmaxf(-e0 / de, t), tc);
                lowerA = eb < 0.0f;          // the second piece lies on the side eb is on
            }
            if (!have_g) g = gap(t, lowerA);
            if (above < 0) above = g >= 0.0f;
            const float gm = gap(tm, lowerA);
            const float gc = tm < tc ? gap(tc, !lowerA) : gm;
            auto crossed = [&](float gg) { return above ? gg <= 0.0f : gg > 0.0f; };
            if (WANT_HIT) { hit.ix = ix; hit.iy = iy; hit.lower = crossed(g) || crossed(gm) ? lowerA : !lowerA; }
            if (crossed(g)) { depth = t; break; }
            if (crossed(gm)) { depth = fmaf(tm - t, g / (g - gm), t); break; }
            if (crossed(gc)) { depth = fmaf(tc - tm, gm / (gm - gc), tm); break; }
            if (tc >= t_hi) break;
            g = gc;
            have_g = true;
            t = tc;
            const int bx0 = ix / L1, by0 = iy / L1;
            if (tx <= ty) ix += sx; else iy += sy;
            if (ix < 0 || iy < 0 || ix > p.W - 2 || iy > p.H - 2) break;
            check_blocks = ix / L1 != bx0 || iy / L1 != by0;
        }
    }
    return depth;
}

}  // namespace terrain_march
