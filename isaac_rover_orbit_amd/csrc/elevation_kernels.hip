// elevation_kernels.hip -- the rolling elevation map from the depth camera (scroll, unproject, reduce, fuse, scan) as one launch
// (gfx950 / CDNA4, wave64).
//
// See include/rover_elevation.h, include/rover_elevation_fill.h and include/rover_elevation_traverse.h for the contracts and the
// operation order.  Five kernels:
//   elevation_step_kernel<G>  one workgroup of 512 threads per env, so the env index -- and with it the pose, the reset flag and
//                             the old origin -- is uniform over the workgroup.  One G x G LDS array of 32-bit words serves three
//                             times: cleared to 0 it takes the frame's keys (pass 1: depth in 16-byte loads where the image and
//                             the ray table start on a 16-byte boundary, four pixels and three ray quads per thread and trip; one
//                             LDS unsigned-max atomic per surviving point); pass 2 walks the slots once, reads the old global
//                             value under the scroll rule, fuses, stores to global and puts the fused float back into the same
//                             LDS word; the scan then looks its columns up in LDS.  A slot is read and written by the same thread
//                             in pass 2, so the map is updated in place without a second copy.
//   elevation_scan_kernel     step 8 alone, the map read from global memory.
//   elevation_fill_kernel<G>  the min-fill of the window and step 8 on the filled window (described at the kernel).
//   elevation_traverse_kernel<G>, elevation_traverse_sparse_kernel<G>  slope, step, roughness and cost of a height window and
//                             step 8 on the cost: for every cell, or only under the scan's columns (at the kernels).
// All run scan_rows(), so they agree on the bits.  The known count is a ballot / popcount per wave into one LDS int per wave,
// summed by thread 0: no atomics on global memory, no float atomics.
// LDS: 4 G^2 bytes of map + 8 wave counters (32 bytes): 65568 bytes at G = 128 (two workgroups per CU), 16416 at G = 64; the
// traverse kernel holds two such images, 131104 bytes at G = 128 (one workgroup per CU).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/rover_hip.h"
#include "../../include/rover_elevation.h"
#include "../../include/rover_elevation_fill.h"
#include "../../include/rover_elevation_traverse.h"
#include "rover_internal.hpp"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int TT = 512;
constexpr int WAVES = TT / 64;
constexpr uint32_t QNAN = 0x7FC00000u;

struct ElevArgs {
    rover_elevation_cfg cfg;
    const float *depth, *ray_b, *pos, *quat, *ray_x, *ray_y;
    const uint8_t *reset_a, *reset_b;
    float *map;                   // the scan kernel only reads it
    int32_t *origin;              // likewise
    float *scan_out;
    uint8_t *known_out;
    int32_t *count_out;
    long long pitch, comp_stride, env_stride, scan_pitch;
    int hw, nx, ny, log_g;
};

struct Pose {
    float px, py, pz, qw, qx, qy, qz;
    bool ok;
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }      // false for a NaN

__device__ __forceinline__ Pose load_pose(const ElevArgs &A, int e)
{
    const float *p = A.pos + (size_t)e * (size_t)A.env_stride, *q = A.quat + (size_t)e * (size_t)A.env_stride;
    const size_t cs = (size_t)A.comp_stride;
    Pose P;
    P.px = p[0]; P.py = p[cs]; P.pz = p[2 * cs];
    P.qw = q[0]; P.qx = q[cs]; P.qy = q[2 * cs]; P.qz = q[3 * cs];
    P.ok = finite_f(P.px) && finite_f(P.py) && finite_f(P.pz) && finite_f(P.qw) && finite_f(P.qx) && finite_f(P.qy) &&
           finite_f(P.qz);
    return P;
}

// the global cell of a finite world coordinate
__device__ __forceinline__ int cell_of(float v, float inv_cell)
{
    return (int)fminf(fmaxf(floorf(__fmul_rn(v, inv_cell)), -1073741824.0f), 1073741824.0f);
}

__device__ __forceinline__ uint32_t key_of(float v)
{
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// one point of pass 1
__device__ __forceinline__ void splat(uint32_t *keys, const ElevArgs &A, const Pose &P, const float (&R)[9], int lo_x, int lo_y,
                                      int G, int log_g, float d, float rx, float ry, float rz)
{
    const rover_elevation_cfg &c = A.cfg;
    if (!(finite_f(d) && d >= c.range_min && d <= c.range_max)) return;
    const float bx = __fadd_rn(c.mount_pos[0], __fmul_rn(d, rx));
    const float by = __fadd_rn(c.mount_pos[1], __fmul_rn(d, ry));
    const float bz = __fadd_rn(c.mount_pos[2], __fmul_rn(d, rz));
    const float wx = __fadd_rn(P.px, __fadd_rn(__fadd_rn(__fmul_rn(R[0], bx), __fmul_rn(R[1], by)), __fmul_rn(R[2], bz)));
    const float wy = __fadd_rn(P.py, __fadd_rn(__fadd_rn(__fmul_rn(R[3], bx), __fmul_rn(R[4], by)), __fmul_rn(R[5], bz)));
    const float wz = __fadd_rn(P.pz, __fadd_rn(__fadd_rn(__fmul_rn(R[6], bx), __fmul_rn(R[7], by)), __fmul_rn(R[8], bz)));
    if (!(finite_f(wx) && finite_f(wy) && finite_f(wz))) return;
    const int gx = cell_of(wx, c.inv_cell), gy = cell_of(wy, c.inv_cell);
    if ((uint32_t)gx - (uint32_t)lo_x >= (uint32_t)G || (uint32_t)gy - (uint32_t)lo_y >= (uint32_t)G) return;
    atomicMax(&keys[((gy & (G - 1)) << log_g) | (gx & (G - 1))], key_of(wz));      // slot < G * G: both terms are masked
}

struct NoDist {};                 // scan_rows' `dist_of` of the step and scan kernels: no fill distance, no bytes written

// What scan_rows makes of a known column's float `h` and byte: the height kernels read (pos.z - h) - height_offset, count the known
// columns and give an unknown column the byte 255; the traverse kernel reads the cost image (CostRead, at its kernel).
struct HeightRead {
    static constexpr uint8_t NO_BYTE = 255;
    static __device__ __forceinline__ float value(const Pose &P, const rover_elevation_cfg &c, float h)
    {
        return __fsub_rn(__fsub_rn(P.pz, h), c.height_offset);
    }
    static __device__ __forceinline__ bool counts(bool known, uint8_t) { return known; }
};

// Step 8 for the env of this workgroup: `load(slot)` is the map's float at a slot < G * G, (cx, cy) the centre of its window.
// With a `dist_of` other than NoDist (the fill and traverse kernels), `dist_row[col]` (where `dist_row` is not NULL) takes
// dist_of(slot, h) of a known column and Read::NO_BYTE of any other.
template <class Load, class DistOf = NoDist, class Read = HeightRead>
__device__ __forceinline__ void scan_rows(const ElevArgs &A, const Pose &P, int e, int G, int log_g, int cx, int cy, bool usable,
                                          int *wave_known, Load load, uint8_t *dist_row = nullptr, DistOf dist_of = DistOf(),
                                          Read = Read())
{
    constexpr bool WITH_DIST = !std::is_same<DistOf, NoDist>::value;
    const rover_elevation_cfg &c = A.cfg;
    const int tid = threadIdx.x, cols = A.nx * A.ny;
    float *row = A.scan_out + (size_t)e * (size_t)A.scan_pitch;
    uint8_t *known_row = A.known_out ? A.known_out + (size_t)e * (size_t)cols : nullptr;
    const int lo_x = cx - (G >> 1), lo_y = cy - (G >> 1);
    float cyaw = 0.0f, syaw = 0.0f;
    if (usable) {
        const float a = __fsub_rn(1.0f, __fmul_rn(2.0f, __fadd_rn(__fmul_rn(P.qy, P.qy), __fmul_rn(P.qz, P.qz))));
        const float b = __fmul_rn(2.0f, __fadd_rn(__fmul_rn(P.qw, P.qz), __fmul_rn(P.qx, P.qy)));
        const float inv = 1.0f / sqrtf(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)));
        cyaw = __fmul_rn(a, inv);
        syaw = __fmul_rn(b, inv);
    }
    int count = 0;                                                   // wave-uniform
    for (int base = tid & ~63; base < cols; base += TT) {            // wave-uniform trip count
        const int col = base + (tid & 63);
        bool known = false, counted = false;
        if (col < cols) {
            float out = c.unknown_value;
            uint8_t dist = Read::NO_BYTE;
            if (usable) {
                const int i = col / A.nx, j = col - i * A.nx;
                const float ox = A.ray_x[j], oy = A.ray_y[i];
                const float x = __fadd_rn(P.px, __fsub_rn(__fmul_rn(cyaw, ox), __fmul_rn(syaw, oy)));
                const float y = __fadd_rn(P.py, __fadd_rn(__fmul_rn(syaw, ox), __fmul_rn(cyaw, oy)));
                if (finite_f(x) && finite_f(y)) {
                    const int gx = cell_of(x, c.inv_cell), gy = cell_of(y, c.inv_cell);
                    if ((uint32_t)gx - (uint32_t)lo_x < (uint32_t)G && (uint32_t)gy - (uint32_t)lo_y < (uint32_t)G) {
                        const int slot = ((gy & (G - 1)) << log_g) | (gx & (G - 1));
                        const float h = load(slot);
                        if (h == h) {
                            known = true;
                            out = Read::value(P, c, h);
                            if constexpr (WITH_DIST) dist = dist_of(slot, h);
                        }
                    }
                }
            }
            row[col] = out;
            if (known_row) known_row[col] = known ? 1 : 0;
            if constexpr (WITH_DIST) {
                if (dist_row) dist_row[col] = dist;
            }
            counted = Read::counts(known, dist);
        }
        count += __popcll(__ballot(counted));
    }
    if (A.count_out) {                                               // kernel argument: uniform over the workgroup
        if ((tid & 63) == 0) wave_known[tid >> 6] = count;
        __syncthreads();
        if (tid == 0) {
            int total = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) total += wave_known[w];
            A.count_out[e] = total;
        }
    }
}

template <int G>
__global__ __launch_bounds__(TT) void elevation_step_kernel(ElevArgs A)
{
    constexpr int LOG_G = G == 8 ? 3 : G == 16 ? 4 : G == 32 ? 5 : G == 64 ? 6 : 7;
    constexpr int CELLS = G * G;
    __shared__ __attribute__((aligned(16))) uint32_t keys[CELLS];
    __shared__ int wave_known[WAVES];
    const rover_elevation_cfg &c = A.cfg;
    const int tid = threadIdx.x, e = blockIdx.x;
    const Pose P = load_pose(A, e);
    const bool reset = (A.reset_a && A.reset_a[e]) || (A.reset_b && A.reset_b[e]);
    float *map = A.map + (size_t)e * CELLS;

    if (!P.ok) {                                                     // uniform over the workgroup
        if (reset)
            for (int s = tid; s < CELLS; s += TT) map[s] = __uint_as_float(QNAN);
        if (A.scan_out) scan_rows(A, P, e, G, LOG_G, 0, 0, false, wave_known, [](int) { return 0.0f; });
        return;
    }
    const int old_x = A.origin[2 * e], old_y = A.origin[2 * e + 1];
    const int cx = cell_of(P.px, c.inv_cell), cy = cell_of(P.py, c.inv_cell);
    const int lo_x = cx - G / 2, lo_y = cy - G / 2;

    for (int s = tid; s < CELLS; s += TT) keys[s] = 0u;
    __syncthreads();

    // ---- pass 1: this frame's points, reduced per cell with the LDS unsigned max
    if (A.depth) {
        const float xx = __fmul_rn(P.qx, P.qx), yy = __fmul_rn(P.qy, P.qy), zz = __fmul_rn(P.qz, P.qz);
        const float xy = __fmul_rn(P.qx, P.qy), xz = __fmul_rn(P.qx, P.qz), yz = __fmul_rn(P.qy, P.qz);
        const float wx = __fmul_rn(P.qw, P.qx), wy = __fmul_rn(P.qw, P.qy), wz = __fmul_rn(P.qw, P.qz);
        const float R[9] = {__fsub_rn(1.0f, __fmul_rn(2.0f, __fadd_rn(yy, zz))), __fmul_rn(2.0f, __fsub_rn(xy, wz)),
                            __fmul_rn(2.0f, __fadd_rn(xz, wy)),
                            __fmul_rn(2.0f, __fadd_rn(xy, wz)), __fsub_rn(1.0f, __fmul_rn(2.0f, __fadd_rn(xx, zz))),
                            __fmul_rn(2.0f, __fsub_rn(yz, wx)),
                            __fmul_rn(2.0f, __fsub_rn(xz, wy)), __fmul_rn(2.0f, __fadd_rn(yz, wx)),
                            __fsub_rn(1.0f, __fmul_rn(2.0f, __fadd_rn(xx, yy)))};
        const float *img = A.depth + (size_t)e * (size_t)A.pitch;
        const int hw = A.hw;
        int done = 0;                                                // pixels the 16-byte path has taken
        if (((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(A.ray_b)) & 15) == 0) {
            const int nq = hw >> 2;
            for (int q = tid; q < nq; q += TT) {
                const v4f d = *reinterpret_cast<const v4f *>(img + 4 * q);
                const v4f *rq = reinterpret_cast<const v4f *>(A.ray_b + 12 * (size_t)q);
                const v4f r0 = rq[0], r1 = rq[1], r2 = rq[2];
                splat(keys, A, P, R, lo_x, lo_y, G, LOG_G, d.x, r0.x, r0.y, r0.z);
                splat(keys, A, P, R, lo_x, lo_y, G, LOG_G, d.y, r0.w, r1.x, r1.y);
                splat(keys, A, P, R, lo_x, lo_y, G, LOG_G, d.z, r1.z, r1.w, r2.x);
                splat(keys, A, P, R, lo_x, lo_y, G, LOG_G, d.w, r2.y, r2.z, r2.w);
            }
            done = 4 * nq;
        }
        for (int k = done + tid; k < hw; k += TT) {
            const float *r = A.ray_b + 3 * (size_t)k;
            splat(keys, A, P, R, lo_x, lo_y, G, LOG_G, img[k], r[0], r[1], r[2]);
        }
    }
    __syncthreads();

    // ---- pass 2: scroll, fuse, store; the fused float goes back into the slot's LDS word
    const int olo_x = old_x - G / 2, olo_y = old_y - G / 2;
    for (int s = tid; s < CELLS; s += TT) {
        const int sx = s & (G - 1), sy = s >> LOG_G;
        // the global cell the slot denotes in the new and in the old window (wrapping arithmetic: equal iff the cells are equal)
        const uint32_t nx_ = (uint32_t)lo_x + (((uint32_t)sx - (uint32_t)lo_x) & (G - 1));
        const uint32_t ny_ = (uint32_t)lo_y + (((uint32_t)sy - (uint32_t)lo_y) & (G - 1));
        const uint32_t ox_ = (uint32_t)olo_x + (((uint32_t)sx - (uint32_t)olo_x) & (G - 1));
        const uint32_t oy_ = (uint32_t)olo_y + (((uint32_t)sy - (uint32_t)olo_y) & (G - 1));
        float v = __uint_as_float(QNAN);
        if (!reset && nx_ == ox_ && ny_ == oy_) v = map[s];
        const uint32_t k = keys[s];
        if (k != 0u) {
            const float f = value_of(k);
            v = (v != v || c.alpha == 1.0f) ? f : __fadd_rn(v, __fmul_rn(c.alpha, __fsub_rn(f, v)));
        }
        if (v != v) v = __uint_as_float(QNAN);
        map[s] = v;
        keys[s] = __float_as_uint(v);
    }
    if (tid == 0) {
        A.origin[2 * e] = cx;
        A.origin[2 * e + 1] = cy;
    }
    if (!A.scan_out) return;                                         // kernel argument: uniform
    __syncthreads();
    scan_rows(A, P, e, G, LOG_G, cx, cy, true, wave_known, [&](int s) { return __uint_as_float(keys[s]); });
}

__global__ __launch_bounds__(TT) void elevation_scan_kernel(ElevArgs A)
{
    __shared__ int wave_known[WAVES];
    const int e = blockIdx.x, G = A.cfg.grid;
    const Pose P = load_pose(A, e);
    const float *map = A.map + ((size_t)e << (2 * A.log_g));
    scan_rows(A, P, e, G, A.log_g, A.origin[2 * e], A.origin[2 * e + 1], P.ok, wave_known, [=](int s) { return map[s]; });
}

// ---- the min-fill (include/rover_elevation_fill.h)
struct FillArgs {
    ElevArgs A;                   // depth, ray_b, reset_*, known_out NULL; map and origin only read
    float *filled_out;
    uint8_t *dist_out, *scan_dist_out;
    int iterations;
};

// One workgroup per env.  LDS: the window's heights (G x G floats) and fill distances (G x G bytes), both in WINDOW order (row i
// over y, column j over x), and two copies of a bit image of the window, one bit per cell and ROWW 32-bit words per row: "this
// cell had a height before the sweep began".  A thread owns a run of RUN consecutive cells of one row, all within one word of
// the bit image.  In sweep k it reads the words over its run, and the last and first bit of the words beside it, for the rows
// i - 1, i, i + 1 of the image of sweep k - 1 (3 to 9 LDS reads, whatever the run's length); OR-ed and widened by one bit to
// either side they say which of its unknown cells have a neighbour that counts, and only those cells (each once in the launch)
// read their neighbours' heights.  No bit is set outside the window, so no sweep tests a bound, and rows of the image do not
// wrap: the seam is no neighbourhood.  The heights and distances are updated in place: a cell written in sweep k has its bit in
// the OTHER image only (the thread ORs this sweep's and the last sweep's new bits into it, which makes it the state after sweep
// k), so readers of sweep k pass over it and one barrier per sweep orders everything.  `last[k & 1] = k` is the vote "sweep k
// filled something": written before barrier k, read behind it, and written again in sweep k + 2 at the earliest.
template <int G>
__global__ __launch_bounds__(TT) void elevation_fill_kernel(FillArgs F)
{
    constexpr int LOG_G = G == 8 ? 3 : G == 16 ? 4 : G == 32 ? 5 : G == 64 ? 6 : 7;
    constexpr int CELLS = G * G, RUN = CELLS >= TT ? CELLS / TT : 1, ROWW = G >= 32 ? G / 32 : 1;
    static_assert(RUN <= 32 && (RUN & (RUN - 1)) == 0 && RUN <= G, "a run lies within one word of one row");
    __shared__ __attribute__((aligned(16))) float hgt[CELLS];
    __shared__ __attribute__((aligned(4))) uint8_t dst[CELLS];
    __shared__ uint32_t had[2][G * ROWW];
    __shared__ int wave_known[WAVES];
    __shared__ int last[2];
    const ElevArgs &A = F.A;
    const int tid = threadIdx.x, e = blockIdx.x;
    const int cx = A.origin[2 * e], cy = A.origin[2 * e + 1];
    const int lo_x = cx - G / 2, lo_y = cy - G / 2;
    const float *map = A.map + (size_t)e * CELLS;

    for (int p = tid; p < 2 * G * ROWW; p += TT) (&had[0][0])[p] = 0u;
    if (tid == 0) last[0] = last[1] = 0;
    for (int s = tid; s < CELLS; s += TT) {                          // slot order in global memory, window order in LDS
        const int j = ((s & (G - 1)) - lo_x) & (G - 1), i = ((s >> LOG_G) - lo_y) & (G - 1);
        const float v = map[s];
        hgt[(i << LOG_G) | j] = v;
        dst[(i << LOG_G) | j] = v != v ? 255 : 0;
    }
    __syncthreads();

    // this thread's run: cells first ... first + RUN - 1 of row i, bits `mine` of word w of that row
    const bool owner = tid * RUN < CELLS;                            // G = 8, 16: fewer cells than threads
    const int first = owner ? tid * RUN : 0, i = first >> LOG_G, j0 = first & (G - 1), w = j0 >> 5;
    const uint32_t mine = (uint32_t)((1ull << RUN) - 1ull) << (j0 & 31);
    uint32_t unknown = 0u;
    if (owner) {
        uint32_t bits = 0u;
#pragma unroll
        for (int r = 0; r < RUN; ++r)
            if (dst[first + r] == 0) bits |= 1u << ((j0 + r) & 31);
        unknown = mine & ~bits;
        if (bits) {
            atomicOr(&had[0][i * ROWW + w], bits);
            atomicOr(&had[1][i * ROWW + w], bits);
        }
    }
    __syncthreads();

    uint32_t fresh = 0u;                                             // the bits this thread set in the sweep before
    for (int k = 1; k <= F.iterations; ++k) {                        // uniform: the bound is an argument, the exit a vote
        const uint32_t *cur = had[(k - 1) & 1];
        uint32_t *next = had[k & 1];
        uint32_t made = 0u;
        if (unknown) {
            // per row i - 1, i, i + 1: bit b + 1 of x[.] is the cell of bit b of word w; bits 0 and 33 are the cells beside the word
            uint64_t x[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int row = i + r - 1;
                uint64_t v = 0;
                if (row >= 0 && row < G) {
                    const uint32_t *rw = cur + row * ROWW;
                    v = (uint64_t)rw[w] << 1;
                    if (ROWW > 1 && w > 0) v |= rw[w - 1] >> 31;
                    if (ROWW > 1 && w < ROWW - 1) v |= (uint64_t)(rw[w + 1] & 1u) << 33;
                }
                x[r] = v;
            }
            const uint64_t any = x[0] | x[1] | x[2];
            for (uint32_t m = unknown & (uint32_t)((any | (any >> 1) | (any >> 2)) & 0xFFFFFFFFu); m != 0u; m &= m - 1u) {
                const int b = __ffs((int)m) - 1, c = (i << LOG_G) | ((w << 5) + b);
                uint32_t best = 0xFFFFFFFFu;                         // above the key of every float that is not a NaN
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const uint32_t t = (uint32_t)(x[r] >> b) & 7u;   // the cells left of, at and right of column b in this row
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        if (t & (1u << q)) best = min(best, key_of(hgt[c + (r - 1) * G + (q - 1)]));
                }
                hgt[c] = value_of(best);
                dst[c] = (uint8_t)k;
                made |= 1u << b;
            }
            unknown &= ~made;
        }
        if (made | fresh) atomicOr(&next[i * ROWW + w], made | fresh);
        fresh = made;
        if (made) last[k & 1] = k;
        __syncthreads();
        if (last[k & 1] != k) break;
    }

    if (F.filled_out || F.dist_out) {                                // kernel arguments: uniform
        float *filled = F.filled_out ? F.filled_out + (size_t)e * CELLS : nullptr;
        uint8_t *dist = F.dist_out ? F.dist_out + (size_t)e * CELLS : nullptr;
        for (int s = tid; s < CELLS; s += TT) {
            const int j = ((s & (G - 1)) - lo_x) & (G - 1), r = ((s >> LOG_G) - lo_y) & (G - 1);
            if (filled) filled[s] = hgt[(r << LOG_G) | j];
            if (dist) dist[s] = dst[(r << LOG_G) | j];
        }
    }
    if (!A.scan_out) return;
    const Pose Q = load_pose(A, e);
    auto at = [=](int s) { return ((((s >> LOG_G) - lo_y) & (G - 1)) << LOG_G) | (((s & (G - 1)) - lo_x) & (G - 1)); };
    scan_rows(A, Q, e, G, LOG_G, cx, cy, Q.ok, wave_known,
              [&](int s) { const int c = at(s); return dst[c] < 255 ? hgt[c] : __uint_as_float(QNAN); },
              F.scan_dist_out ? F.scan_dist_out + (size_t)e * (size_t)(A.nx * A.ny) : nullptr, [&](int s, float) { return dst[at(s)]; });
}

// ---- slope, step, roughness and cost (include/rover_elevation_traverse.h)
struct TraverseArgs {
    ElevArgs A;                   // depth, ray_b, reset_*, known_out NULL; map (the heights) and origin only read; cfg.unknown_value
                                  // holds unknown_cost, scan_out the cost scan, count_out the lethal count
    rover_elevation_traverse_cfg t;
    uint8_t *class_out;
    float *slope_out, *step_out, *rough_out, *cost_out;
};

// The cost image holds a cell's verdict in one float: NaN = no verdict (class 0), the cost (<= 1) of a class-1 cell, and LETHAL,
// which no cost can be, for a class-2 cell, whose cost is 1.
constexpr float LETHAL = 2.0f;

struct CostRead {                 // scan_rows' Read over the cost image: the cost itself, class 0 for no column, the class-2 count
    static constexpr uint8_t NO_BYTE = 0;
    static __device__ __forceinline__ float value(const Pose &, const rover_elevation_cfg &, float v) { return fminf(v, 1.0f); }
    static __device__ __forceinline__ bool counts(bool, uint8_t cls) { return cls == 2; }
};

__device__ __forceinline__ float one_sided(float lo, float mid, float hi, float inv_cell)
{
    const bool l = finite_f(lo), u = finite_f(hi);
    if (l && u) return __fmul_rn(__fsub_rn(hi, lo), __fmul_rn(0.5f, inv_cell));
    if (u) return __fmul_rn(__fsub_rn(hi, mid), inv_cell);
    if (l) return __fmul_rn(__fsub_rn(mid, lo), inv_cell);
    return 0.0f;
}

// Step 2 and 3 of the header for the CH cells (i, j0) ... (i, j0 + CH - 1) of the window image `hgt`, all inside the window.  Per
// neighbourhood row the strip of CH + 2 R heights over the cells is read from LDS once and every cell takes its 2 R + 1 of them
// from registers; a cell's accumulation order is the header's (di outer, dj inner) whatever CH is, so a cell's bits do not depend
// on who computes it, or with which neighbours.  `verdict` takes the image's float (see LETHAL); a layer of a cell without a
// verdict is the quiet NaN.
template <int G, int CH, int R>
__device__ __forceinline__ void traverse_cells(const float *hgt, const rover_elevation_cfg &c, const rover_elevation_traverse_cfg &t,
                                               int i, int j0, float (&slope)[CH], float (&step)[CH], float (&rough)[CH],
                                               float (&verdict)[CH])
{
    constexpr int LOG_G = G == 8 ? 3 : G == 16 ? 4 : G == 32 ? 5 : G == 64 ? 6 : 7;
    const float nan = __uint_as_float(QNAN);
    auto at = [&](int row, int col) {                                // outside the window nothing is usable
        return ((uint32_t)row < (uint32_t)G && (uint32_t)col < (uint32_t)G) ? hgt[(row << LOG_G) | col] : nan;
    };
    float hc[CH + 2], gx[CH], gy[CH], acc[CH];
    uint32_t kmin[CH], kmax[CH];
    int support[CH];
#pragma unroll
    for (int q = 0; q < CH + 2; ++q) hc[q] = at(i, j0 - 1 + q);
#pragma unroll
    for (int q = 0; q < CH; ++q) {
        gx[q] = one_sided(hc[q], hc[q + 1], hc[q + 2], c.inv_cell);
        gy[q] = one_sided(at(i - 1, j0 + q), hc[q + 1], at(i + 1, j0 + q), c.inv_cell);
        acc[q] = 0.0f;
        kmin[q] = 0xFFFFFFFFu;
        kmax[q] = 0u;
        support[q] = 0;
    }
    for (int di = -R; di <= R; ++di) {
        const int row = i + di;
        if ((uint32_t)row >= (uint32_t)G) continue;
        float s[CH + 2 * R];
#pragma unroll
        for (int q = 0; q < CH + 2 * R; ++q) s[q] = at(row, j0 - R + q);
        const float dy = __fmul_rn((float)di, c.cell);
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            const float along_y = __fmul_rn(gy[q], dy);
#pragma unroll
            for (int dj = -R; dj <= R; ++dj) {
                const float h = s[q + dj + R];
                if (!finite_f(h)) continue;
                const uint32_t k = key_of(h);
                kmin[q] = min(kmin[q], k);
                kmax[q] = max(kmax[q], k);
                ++support[q];
                if (dj != 0 || di != 0) {
                    const float res = __fsub_rn(__fsub_rn(h, hc[q + 1]),
                                                __fadd_rn(__fmul_rn(gx[q], __fmul_rn((float)dj, c.cell)), along_y));
                    acc[q] = __fadd_rn(acc[q], __fmul_rn(res, res));
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < CH; ++q) {
        const bool none = !finite_f(hc[q + 1]) || support[q] < t.min_support;      // then what follows is computed and dropped
        const float sl = sqrtf(__fadd_rn(__fmul_rn(gx[q], gx[q]), __fmul_rn(gy[q], gy[q])));
        const float st = __fsub_rn(value_of(kmax[q]), value_of(kmin[q]));
        const int cnt = support[q] - 1;
        const float ro = cnt == 0 ? 0.0f : sqrtf(acc[q] / (float)cnt);
        const bool lethal = !(sl < t.slope_crit && st < t.step_crit && ro < t.rough_crit);
        const float cost = fminf(__fadd_rn(__fadd_rn(__fmul_rn(t.w_slope, sl / t.slope_crit), __fmul_rn(t.w_step, st / t.step_crit)),
                                           __fmul_rn(t.w_rough, ro / t.rough_crit)), 1.0f);
        const uint32_t keep = none ? 0u : 0xFFFFFFFFu;              // each element assigned once: the arrays stay in registers
        slope[q] = __uint_as_float((__float_as_uint(sl) & keep) | (QNAN & ~keep));
        step[q] = __uint_as_float((__float_as_uint(st) & keep) | (QNAN & ~keep));
        rough[q] = __uint_as_float((__float_as_uint(ro) & keep) | (QNAN & ~keep));
        verdict[q] = __uint_as_float((__float_as_uint(lethal ? LETHAL : cost) & keep) | (QNAN & ~keep));
    }
}

template <int G, int CH>
__device__ __forceinline__ void traverse_chunk(const float *hgt, const rover_elevation_cfg &c, const rover_elevation_traverse_cfg &t,
                                               int i, int j0, float (&slope)[CH], float (&step)[CH], float (&rough)[CH],
                                               float (&verdict)[CH])
{
    switch (t.radius) {                                              // a kernel argument: uniform
    case 1:  traverse_cells<G, CH, 1>(hgt, c, t, i, j0, slope, step, rough, verdict); break;
    case 2:  traverse_cells<G, CH, 2>(hgt, c, t, i, j0, slope, step, rough, verdict); break;
    case 3:  traverse_cells<G, CH, 3>(hgt, c, t, i, j0, slope, step, rough, verdict); break;
    default: traverse_cells<G, CH, 4>(hgt, c, t, i, j0, slope, step, rough, verdict); break;
    }
}

// ---- the two traverse kernels, one workgroup per env; both load the window as the fill does
template <int G>
__device__ __forceinline__ void load_window(const ElevArgs &A, int e, int lo_x, int lo_y, float *hgt)
{
    constexpr int LOG_G = G == 8 ? 3 : G == 16 ? 4 : G == 32 ? 5 : G == 64 ? 6 : 7;
    const float *map = A.map + (size_t)e * (G * G);
    for (int s = threadIdx.x; s < G * G; s += TT) {                  // slot order in global memory, window order in LDS
        const int j = ((s & (G - 1)) - lo_x) & (G - 1), i = ((s >> LOG_G) - lo_y) & (G - 1);
        hgt[(i << LOG_G) | j] = map[s];
    }
    __syncthreads();
}

__device__ __forceinline__ uint8_t class_of(int, float v) { return (uint8_t)(v > 1.0f ? 2 : 1); }      // of a verdict that is no NaN

// The dense form, launched when a window output is asked for.  LDS: the window's heights and the cost image (see LETHAL), G x G
// floats each, both in WINDOW order.  A thread owns a run of RUN consecutive cells of one row, as in the fill, and takes them CH
// at a time through traverse_cells: 8 at G = 64, where the strip slides along the whole run, and at G = 128, where it slides
// along each quarter of it (the per-cell accumulators of 32 cells would not fit the registers); 1 below (at G = 32 a run is two
// cells; hipcc 7.2's instruction selection crashes on chunks of two and of four cells).  The thread writes its cells' layers to
// global memory itself, in slot order (a run is contiguous there but for the seam), and the verdicts into the cost image, which
// the scan reads behind one barrier.
template <int G>
__global__ __launch_bounds__(TT) void elevation_traverse_kernel(TraverseArgs F)
{
    constexpr int LOG_G = G == 8 ? 3 : G == 16 ? 4 : G == 32 ? 5 : G == 64 ? 6 : 7;
    constexpr int CELLS = G * G, RUN = CELLS >= TT ? CELLS / TT : 1, CH = RUN < 8 ? 1 : 8;
    static_assert(RUN <= G && RUN % CH == 0, "a run lies within one row and is whole chunks");
    __shared__ __attribute__((aligned(16))) float hgt[CELLS];
    __shared__ __attribute__((aligned(16))) float cst[CELLS];
    __shared__ int wave_known[WAVES];
    const ElevArgs &A = F.A;
    const int tid = threadIdx.x, e = blockIdx.x;
    const int cx = A.origin[2 * e], cy = A.origin[2 * e + 1];
    const int lo_x = cx - G / 2, lo_y = cy - G / 2;
    load_window<G>(A, e, lo_x, lo_y, hgt);

    if (tid * RUN < CELLS) {                                         // G = 8, 16: fewer cells than threads
        const size_t base = (size_t)e * CELLS;
        const int first = tid * RUN, i = first >> LOG_G, slot_row = ((lo_y + i) & (G - 1)) << LOG_G;
        for (int j0 = first & (G - 1), end = j0 + RUN; j0 < end; j0 += CH) {
            float slope[CH], step[CH], rough[CH], verdict[CH];
            traverse_chunk<G, CH>(hgt, A.cfg, F.t, i, j0, slope, step, rough, verdict);
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const size_t s = base + (size_t)(slot_row | ((lo_x + j0 + q) & (G - 1)));
                const float v = verdict[q];
                cst[(i << LOG_G) | (j0 + q)] = v;
                if (F.slope_out) F.slope_out[s] = slope[q];
                if (F.step_out) F.step_out[s] = step[q];
                if (F.rough_out) F.rough_out[s] = rough[q];
                if (F.cost_out) F.cost_out[s] = v != v ? v : fminf(v, 1.0f);
            }
        }
    }
    if (!A.scan_out) return;                                         // kernel argument: uniform
    __syncthreads();
    const Pose Q = load_pose(A, e);
    auto at = [=](int s) { return ((((s >> LOG_G) - lo_y) & (G - 1)) << LOG_G) | (((s & (G - 1)) - lo_x) & (G - 1)); };
    scan_rows(A, Q, e, G, LOG_G, cx, cy, Q.ok, wave_known, [&](int s) { return cst[at(s)]; },
              F.class_out ? F.class_out + (size_t)e * (size_t)(A.nx * A.ny) : nullptr, class_of, CostRead());
}

// The sparse form, launched when no window output is asked for: only the cells under the scan's columns need a verdict, at most
// nx * ny of the G x G.  Each column computes its cell's with CH = 1 through the same device function, so the bits are the dense
// form's; there is no cost image, and the few registers of the one-cell form leave room for several workgroups per CU.
template <int G>
__global__ __launch_bounds__(TT) void elevation_traverse_sparse_kernel(TraverseArgs F)
{
    constexpr int LOG_G = G == 8 ? 3 : G == 16 ? 4 : G == 32 ? 5 : G == 64 ? 6 : 7;
    __shared__ __attribute__((aligned(16))) float hgt[G * G];
    __shared__ int wave_known[WAVES];
    const ElevArgs &A = F.A;
    const int e = blockIdx.x;
    const int cx = A.origin[2 * e], cy = A.origin[2 * e + 1];
    const int lo_x = cx - G / 2, lo_y = cy - G / 2;
    load_window<G>(A, e, lo_x, lo_y, hgt);
    const Pose Q = load_pose(A, e);
    scan_rows(A, Q, e, G, LOG_G, cx, cy, Q.ok, wave_known,
              [&](int s) {
                  const int i = ((s >> LOG_G) - lo_y) & (G - 1), j = ((s & (G - 1)) - lo_x) & (G - 1);
                  float slope[1], step[1], rough[1], verdict[1];
                  traverse_chunk<G, 1>(hgt, A.cfg, F.t, i, j, slope, step, rough, verdict);
                  return verdict[0];
              },
              F.class_out ? F.class_out + (size_t)e * (size_t)(A.nx * A.ny) : nullptr, class_of, CostRead());
}

bool pos_ok(float v) { return std::isfinite(v) && v > 0.0f; }

bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y ? y - x < a_bytes : x - y < b_bytes;
}

// the checks both entry points share; `who` names the entry point in the message
int check_common(const char *who, const rover_elevation_cfg *cfg, const float *pos, const float *quat, int64_t comp_stride,
                 int64_t env_stride, const float *map, const int32_t *origin, const float *ray_x, int32_t nx, const float *ray_y,
                 int32_t ny, const float *scan_out, int64_t scan_pitch, const int32_t *count_out, int32_t n)
{
    auto refuse = [who](const char *why) {
        rover_internal_fail(ROVER_ERR_INVALID, who, why);
        return ROVER_ERR_INVALID;
    };
    auto unsupported = [who](const char *why) {
        rover_internal_fail(ROVER_ERR_UNSUPPORTED, who, why);
        return ROVER_ERR_UNSUPPORTED;
    };
    if (!cfg || !pos || !quat || !map || !origin || !ray_x || !ray_y) return refuse("NULL argument");
    if (n <= 0) return refuse("n must be > 0");
    const int g = cfg->grid;
    if (g < ROVER_ELEVATION_MIN_GRID || g > ROVER_ELEVATION_MAX_GRID || (g & (g - 1)) != 0)
        return unsupported("grid must be a power of two in [8, 128]");
    if (nx <= 0 || ny <= 0) return refuse("nx and ny must be > 0");
    if ((int64_t)nx * (int64_t)ny > ROVER_ELEVATION_MAX_RAYS) return unsupported("nx * ny must be <= 4096");
    if (comp_stride <= 0 || env_stride <= 0) return refuse("comp_stride and env_stride must be > 0");
    if ((reinterpret_cast<uintptr_t>(pos) | reinterpret_cast<uintptr_t>(quat) | reinterpret_cast<uintptr_t>(map) |
         reinterpret_cast<uintptr_t>(origin) | reinterpret_cast<uintptr_t>(ray_x) | reinterpret_cast<uintptr_t>(ray_y) |
         reinterpret_cast<uintptr_t>(scan_out) | reinterpret_cast<uintptr_t>(count_out)) & 3)
        return refuse("float and int32 pointers must be 4-byte aligned");
    if (scan_out && scan_pitch < (int64_t)nx * (int64_t)ny) return refuse("scan_pitch must be >= nx * ny");
    if (scan_out && scan_pitch > (INT64_MAX / 8) / (int64_t)n) return refuse("n * scan_pitch is out of range");
    const rover_elevation_cfg &c = *cfg;
    if (!pos_ok(c.cell) || !pos_ok(c.inv_cell)) return refuse("cell and inv_cell must be finite and > 0");
    if (!pos_ok(c.range_min)) return refuse("range_min must be finite and > 0");
    if (!(c.range_max >= c.range_min)) return refuse("range_max must be >= range_min");
    if (!(c.alpha > 0.0f && c.alpha <= 1.0f)) return refuse("alpha must be in (0, 1]");
    if (c.unknown_value != c.unknown_value) return refuse("unknown_value must not be a NaN");
    if (c.height_offset != c.height_offset) return refuse("height_offset must not be a NaN");
    if (!(std::isfinite(c.mount_pos[0]) && std::isfinite(c.mount_pos[1]) && std::isfinite(c.mount_pos[2])))
        return refuse("mount_pos must be finite");
    if (scan_out) {
        const uint64_t map_bytes = (uint64_t)n * (uint64_t)g * (uint64_t)g * 4u;
        const uint64_t scan_bytes = ((uint64_t)(n - 1) * (uint64_t)scan_pitch + (uint64_t)nx * (uint64_t)ny) * 4u;
        if (overlap(map, map_bytes, scan_out, scan_bytes)) return refuse("map and scan_out overlap");
    }
    return ROVER_OK;
}

int log2_of(int g)
{
    int l = 0;
    while ((1 << l) < g) ++l;
    return l;
}

}  // namespace

extern "C" {

size_t rover_elevation_cfg_bytes(void) { return sizeof(rover_elevation_cfg); }

int rover_elevation_step(const rover_elevation_cfg *cfg, const float *depth, int64_t pitch_floats, int32_t height, int32_t width,
                         const float *ray_b, const float *pos, const float *quat, int64_t comp_stride, int64_t env_stride,
                         const uint8_t *reset_a, const uint8_t *reset_b, float *map, int32_t *origin, const float *ray_x,
                         int32_t nx, const float *ray_y, int32_t ny, float *scan_out, int64_t scan_pitch, uint8_t *known_out,
                         int32_t *count_out, int32_t n, void *stream)
{
    static const char who[] = "rover_elevation_step: %s";
    auto refuse = [](const char *why) { return rover_internal_fail(ROVER_ERR_INVALID, who, why); };
    if (int rc = check_common(who, cfg, pos, quat, comp_stride, env_stride, map, origin, ray_x, nx, ray_y, ny, scan_out, scan_pitch,
                              count_out, n))
        return rc;
    if (depth && !ray_b) return refuse("NULL argument (depth needs ray_b)");
    if (height <= 0 || width <= 0) return refuse("height and width must be > 0");
    const int64_t hw = (int64_t)height * (int64_t)width;
    if (hw > ROVER_ELEVATION_MAX_PIXELS) return rover_internal_fail(ROVER_ERR_UNSUPPORTED, who, "height * width must be <= 16384");
    if ((reinterpret_cast<uintptr_t>(depth) | reinterpret_cast<uintptr_t>(ray_b)) & 3)
        return refuse("float and int32 pointers must be 4-byte aligned");
    if (depth) {
        if (pitch_floats < hw) return refuse("pitch_floats must be >= height * width");
        if (pitch_floats > (INT64_MAX / 8) / (int64_t)n) return refuse("n * pitch_floats is out of range");
        const uint64_t map_bytes = (uint64_t)n * (uint64_t)cfg->grid * (uint64_t)cfg->grid * 4u;
        const uint64_t depth_bytes = ((uint64_t)(n - 1) * (uint64_t)pitch_floats + (uint64_t)hw) * 4u;
        if (overlap(map, map_bytes, depth, depth_bytes)) return refuse("map and depth overlap");
    }
    int dev;
    if (int rc = device_of(map, &dev, true)) return rc;
    DeviceGuard guard(dev);
    ElevArgs A;
    A.cfg = *cfg;
    A.depth = depth; A.ray_b = ray_b; A.pos = pos; A.quat = quat; A.ray_x = ray_x; A.ray_y = ray_y;
    A.reset_a = reset_a; A.reset_b = reset_b;
    A.map = map; A.origin = origin;
    A.scan_out = scan_out; A.known_out = known_out; A.count_out = count_out;
    A.pitch = (long long)pitch_floats; A.comp_stride = (long long)comp_stride; A.env_stride = (long long)env_stride;
    A.scan_pitch = (long long)scan_pitch;
    A.hw = (int)hw; A.nx = nx; A.ny = ny; A.log_g = log2_of(cfg->grid);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (cfg->grid) {
    case 8:   hipLaunchKernelGGL(elevation_step_kernel<8>, dim3((unsigned)n), dim3(TT), 0, st, A); break;
    case 16:  hipLaunchKernelGGL(elevation_step_kernel<16>, dim3((unsigned)n), dim3(TT), 0, st, A); break;
    case 32:  hipLaunchKernelGGL(elevation_step_kernel<32>, dim3((unsigned)n), dim3(TT), 0, st, A); break;
    case 64:  hipLaunchKernelGGL(elevation_step_kernel<64>, dim3((unsigned)n), dim3(TT), 0, st, A); break;
    default:  hipLaunchKernelGGL(elevation_step_kernel<128>, dim3((unsigned)n), dim3(TT), 0, st, A); break;
    }
    return launched("elevation_step_kernel launch: %s");
}

int rover_elevation_scan(const rover_elevation_cfg *cfg, const float *pos, const float *quat, int64_t comp_stride,
                         int64_t env_stride, const float *map, const int32_t *origin, const float *ray_x, int32_t nx,
                         const float *ray_y, int32_t ny, float *scan_out, int64_t scan_pitch, uint8_t *known_out,
                         int32_t *count_out, int32_t n, void *stream)
{
    static const char who[] = "rover_elevation_scan: %s";
    if (!scan_out) return rover_internal_fail(ROVER_ERR_INVALID, who, "NULL argument");
    if (int rc = check_common(who, cfg, pos, quat, comp_stride, env_stride, map, origin, ray_x, nx, ray_y, ny, scan_out, scan_pitch,
                              count_out, n))
        return rc;
    int dev;
    if (int rc = device_of(map, &dev, true)) return rc;
    DeviceGuard guard(dev);
    ElevArgs A;
    A.cfg = *cfg;
    A.depth = nullptr; A.ray_b = nullptr; A.pos = pos; A.quat = quat; A.ray_x = ray_x; A.ray_y = ray_y;
    A.reset_a = nullptr; A.reset_b = nullptr;
    A.map = const_cast<float *>(map); A.origin = const_cast<int32_t *>(origin);
    A.scan_out = scan_out; A.known_out = known_out; A.count_out = count_out;
    A.pitch = 0; A.comp_stride = (long long)comp_stride; A.env_stride = (long long)env_stride;
    A.scan_pitch = (long long)scan_pitch;
    A.hw = 0; A.nx = nx; A.ny = ny; A.log_g = log2_of(cfg->grid);
    hipLaunchKernelGGL(elevation_scan_kernel, dim3((unsigned)n), dim3(TT), 0, static_cast<hipStream_t>(stream), A);
    return launched("elevation_scan_kernel launch: %s");
}

size_t rover_elevation_fill_cfg_bytes(void) { return sizeof(rover_elevation_fill_cfg); }

int rover_elevation_fill(const rover_elevation_cfg *cfg, const rover_elevation_fill_cfg *fill, const float *pos, const float *quat,
                         int64_t comp_stride, int64_t env_stride, const float *map, const int32_t *origin, const float *ray_x,
                         int32_t nx, const float *ray_y, int32_t ny, float *scan_out, int64_t scan_pitch, uint8_t *scan_dist_out,
                         int32_t *count_out, float *filled_out, uint8_t *dist_out, int32_t n, void *stream)
{
    static const char who[] = "rover_elevation_fill: %s";
    auto refuse = [](const char *why) { return rover_internal_fail(ROVER_ERR_INVALID, who, why); };
    if (!fill) return refuse("NULL argument");
    if (!scan_out && !filled_out) return refuse("NULL argument (one of scan_out and filled_out is required)");
    if (!scan_out && map) {                                          // no scan: the ray tables are not read and may be NULL
        ray_x = ray_x ? ray_x : map;
        ray_y = ray_y ? ray_y : map;
    }
    if (int rc = check_common(who, cfg, pos, quat, comp_stride, env_stride, map, origin, ray_x, nx, ray_y, ny, scan_out, scan_pitch,
                              count_out, n))
        return rc;
    if (fill->iterations < 1 || fill->iterations > ROVER_ELEVATION_FILL_MAX_ITERATIONS) return refuse("iterations must be in [1, 254]");
    if (reinterpret_cast<uintptr_t>(filled_out) & 3) return refuse("float and int32 pointers must be 4-byte aligned");
    if (filled_out) {
        const uint64_t map_bytes = (uint64_t)n * (uint64_t)cfg->grid * (uint64_t)cfg->grid * 4u;
        if (overlap(map, map_bytes, filled_out, map_bytes)) return refuse("map and filled_out overlap");
        if (scan_out) {
            const uint64_t scan_bytes = ((uint64_t)(n - 1) * (uint64_t)scan_pitch + (uint64_t)nx * (uint64_t)ny) * 4u;
            if (overlap(filled_out, map_bytes, scan_out, scan_bytes)) return refuse("filled_out and scan_out overlap");
        }
    }
    int dev;
    if (int rc = device_of(map, &dev, true)) return rc;
    DeviceGuard guard(dev);
    FillArgs F;
    ElevArgs &A = F.A;
    A.cfg = *cfg;
    A.depth = nullptr; A.ray_b = nullptr; A.pos = pos; A.quat = quat; A.ray_x = ray_x; A.ray_y = ray_y;
    A.reset_a = nullptr; A.reset_b = nullptr;
    A.map = const_cast<float *>(map); A.origin = const_cast<int32_t *>(origin);
    A.scan_out = scan_out; A.known_out = nullptr; A.count_out = scan_out ? count_out : nullptr;
    A.pitch = 0; A.comp_stride = (long long)comp_stride; A.env_stride = (long long)env_stride;
    A.scan_pitch = (long long)scan_pitch;
    A.hw = 0; A.nx = nx; A.ny = ny; A.log_g = log2_of(cfg->grid);
    F.filled_out = filled_out; F.dist_out = dist_out; F.scan_dist_out = scan_out ? scan_dist_out : nullptr;
    F.iterations = fill->iterations;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (cfg->grid) {
    case 8:   hipLaunchKernelGGL(elevation_fill_kernel<8>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
    case 16:  hipLaunchKernelGGL(elevation_fill_kernel<16>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
    case 32:  hipLaunchKernelGGL(elevation_fill_kernel<32>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
    case 64:  hipLaunchKernelGGL(elevation_fill_kernel<64>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
    default:  hipLaunchKernelGGL(elevation_fill_kernel<128>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
    }
    return launched("elevation_fill_kernel launch: %s");
}

size_t rover_elevation_traverse_cfg_bytes(void) { return sizeof(rover_elevation_traverse_cfg); }

int rover_elevation_traverse(const rover_elevation_cfg *cfg, const rover_elevation_traverse_cfg *t, const float *pos,
                             const float *quat, int64_t comp_stride, int64_t env_stride, const float *heights, const int32_t *origin,
                             const float *ray_x, int32_t nx, const float *ray_y, int32_t ny, float *cost_scan_out, int64_t scan_pitch,
                             uint8_t *class_out, int32_t *lethal_count_out, float *slope_out, float *step_out, float *rough_out,
                             float *cost_out, int32_t n, void *stream)
{
    static const char who[] = "rover_elevation_traverse: %s";
    auto refuse = [](const char *why) { return rover_internal_fail(ROVER_ERR_INVALID, who, why); };
    float *const layers[4] = {slope_out, step_out, rough_out, cost_out};
    if (!t) return refuse("NULL argument");
    if (!cost_scan_out && !slope_out && !step_out && !rough_out && !cost_out)
        return refuse("NULL argument (cost_scan_out or one of the four window outputs is required)");
    if (!cost_scan_out && heights) {                                 // no scan: the ray tables are not read and may be NULL
        ray_x = ray_x ? ray_x : heights;
        ray_y = ray_y ? ray_y : heights;
    }
    if (int rc = check_common(who, cfg, pos, quat, comp_stride, env_stride, heights, origin, ray_x, nx, ray_y, ny, cost_scan_out,
                              scan_pitch, lethal_count_out, n))
        return rc;
    if (t->radius < 1 || t->radius > ROVER_ELEVATION_TRAVERSE_MAX_RADIUS) return refuse("radius must be in [1, 4]");
    const int side = 2 * t->radius + 1;
    if (t->min_support < 1 || t->min_support > side * side) return refuse("min_support must be in [1, (2 radius + 1)^2]");
    if (!pos_ok(t->slope_crit) || !pos_ok(t->step_crit) || !pos_ok(t->rough_crit))
        return refuse("slope_crit, step_crit and rough_crit must be finite and > 0");
    for (float w : {t->w_slope, t->w_step, t->w_rough})
        if (!(std::isfinite(w) && w >= 0.0f)) return refuse("w_slope, w_step and w_rough must be finite and >= 0");
    {
        volatile float two = t->w_slope + t->w_step;                 // each sum rounded to fp32, in this order
        volatile float sum = two + t->w_rough;
        if (!(sum <= 1.0f)) return refuse("the weights' sum (w_slope + w_step) + w_rough must be <= 1");
    }
    if (t->unknown_cost != t->unknown_cost) return refuse("unknown_cost must not be a NaN");
    const uint64_t cells_bytes = (uint64_t)n * (uint64_t)cfg->grid * (uint64_t)cfg->grid * 4u;
    for (float *p : layers) {
        if (reinterpret_cast<uintptr_t>(p) & 3) return refuse("float and int32 pointers must be 4-byte aligned");
        if (p && overlap(heights, cells_bytes, p, cells_bytes)) return refuse("heights and a window output overlap");
    }
    if (cost_scan_out) {                                             // heights and cost_scan_out: check_common
        const uint64_t cols = (uint64_t)nx * (uint64_t)ny;
        if (class_out && overlap(heights, cells_bytes, class_out, (uint64_t)n * cols)) return refuse("heights and class_out overlap");
        if (lethal_count_out && overlap(heights, cells_bytes, lethal_count_out, (uint64_t)n * 4u))
            return refuse("heights and lethal_count_out overlap");
    }
    int dev;
    if (int rc = device_of(heights, &dev, true)) return rc;
    DeviceGuard guard(dev);
    TraverseArgs F;
    ElevArgs &A = F.A;
    A.cfg = *cfg;
    A.cfg.unknown_value = t->unknown_cost;                           // what scan_rows gives a column without a cost
    A.depth = nullptr; A.ray_b = nullptr; A.pos = pos; A.quat = quat; A.ray_x = ray_x; A.ray_y = ray_y;
    A.reset_a = nullptr; A.reset_b = nullptr;
    A.map = const_cast<float *>(heights); A.origin = const_cast<int32_t *>(origin);
    A.scan_out = cost_scan_out; A.known_out = nullptr; A.count_out = cost_scan_out ? lethal_count_out : nullptr;
    A.pitch = 0; A.comp_stride = (long long)comp_stride; A.env_stride = (long long)env_stride;
    A.scan_pitch = (long long)scan_pitch;
    A.hw = 0; A.nx = nx; A.ny = ny; A.log_g = log2_of(cfg->grid);
    F.t = *t;
    F.class_out = cost_scan_out ? class_out : nullptr;
    F.slope_out = slope_out; F.step_out = step_out; F.rough_out = rough_out; F.cost_out = cost_out;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!slope_out && !step_out && !rough_out && !cost_out) {        // the scan alone: verdicts only under its columns
        switch (cfg->grid) {
        case 8:   hipLaunchKernelGGL(elevation_traverse_sparse_kernel<8>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
        case 16:  hipLaunchKernelGGL(elevation_traverse_sparse_kernel<16>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
        case 32:  hipLaunchKernelGGL(elevation_traverse_sparse_kernel<32>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
        case 64:  hipLaunchKernelGGL(elevation_traverse_sparse_kernel<64>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
        default:  hipLaunchKernelGGL(elevation_traverse_sparse_kernel<128>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
        }
        return launched("elevation_traverse_sparse_kernel launch: %s");
    }
    switch (cfg->grid) {
    case 8:   hipLaunchKernelGGL(elevation_traverse_kernel<8>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
    case 16:  hipLaunchKernelGGL(elevation_traverse_kernel<16>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
    case 32:  hipLaunchKernelGGL(elevation_traverse_kernel<32>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
    case 64:  hipLaunchKernelGGL(elevation_traverse_kernel<64>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
    default:  hipLaunchKernelGGL(elevation_traverse_kernel<128>, dim3((unsigned)n), dim3(TT), 0, st, F); break;
    }
    return launched("elevation_traverse_kernel launch: %s");
}

}  // extern "C"
