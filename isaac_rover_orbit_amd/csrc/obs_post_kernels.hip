// obs_post_kernels.hip -- ORBIT's observation post-processing (noise -> clip -> scale) in place, one launch (gfx950 / CDNA4, wave64).
//
// See include/rover_obs_post.h for the contract and the draw addressing.  One kernel:
//   obs_post_kernel   a thread owns one Philox quad of one row: the four absolute columns 4 q .. 4 q + 3.  It finds which of them
//                     a segment covers, reads those (one 16-byte access when all four are covered and the address is 16-byte
//                     aligned, otherwise dword by dword: an observation row is 3860 bytes, so three rows in four are not aligned),
//                     draws its four Philox words once, walks the segments (a wave-uniform loop over the kernel arguments) and
//                     writes the same columns back.  Columns outside every segment are neither read nor written.
// Only the quads [q0, q0 + nq) that a segment reaches get a thread.  No LDS, no atomics, nothing shared between threads.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/rover_hip.h"
#include "../../include/rover_obs_post.h"
#include "rover_internal.hpp"
#include "train_math.hpp"   // philox4x32, unit_uniform, box_muller, tclamp

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int TT = 256;
constexpr long long MAX_BLOCKS = 1 << 20;

struct PostArgs {
    rover_obs_post_segment seg[ROVER_OBS_POST_MAX_SEGMENTS];
    float *rows;
    long long pitch;              // floats between two rows
    unsigned long long total;     // n * nq threads of work
    unsigned long long id0;       // env_id_offset
    int n_seg, width, q0, nq;     // the quads [q0, q0 + nq) of a row
    uint32_t k0, k1, c1, c2, tag;
    int draws;                    // some segment is uniform or gaussian
};

__global__ __launch_bounds__(TT) void obs_post_kernel(PostArgs A)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * TT;
    for (unsigned long long t = (unsigned long long)blockIdx.x * TT + threadIdx.x; t < A.total; t += stride) {
        // (row, quad) of this thread; a 32-bit division where the launch is small enough for one
        unsigned long long row;
        int q;
        if (A.total <= 0xFFFFFFFFull) {
            const uint32_t r32 = (uint32_t)t / (uint32_t)A.nq;
            row = r32;
            q = A.q0 + (int)((uint32_t)t - r32 * (uint32_t)A.nq);
        } else {
            row = t / (unsigned long long)A.nq;
            q = A.q0 + (int)(t - row * (unsigned long long)A.nq);
        }
        const int col = 4 * q;
        // which of the four columns a segment covers (segments do not overlap and stay inside the row)
        unsigned mask = 0;
        for (int s = 0; s < A.n_seg; ++s) {
            const int lo = A.seg[s].col_lo, hi = A.seg[s].col_hi;
#pragma unroll
            for (int j = 0; j < 4; ++j) mask |= (col + j >= lo && col + j < hi) ? 1u << j : 0u;
        }
        if (mask == 0) continue;
        float *p = A.rows + (size_t)row * (size_t)A.pitch + col;
        const bool vec = mask == 0xFu && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (vec) {
            const v4f x = *reinterpret_cast<const v4f *>(p);
            v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (mask & (1u << j)) v[j] = p[j];
        }
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (A.draws) philox4x32((uint32_t)(A.id0 + row), A.c1, A.c2, A.tag | (uint32_t)q, A.k0, A.k1, w);
        for (int s = 0; s < A.n_seg; ++s) {
            const rover_obs_post_segment S = A.seg[s];
            unsigned in = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) in |= (col + j >= S.col_lo && col + j < S.col_hi) ? 1u << j : 0u;
            if (in == 0) continue;
            if (S.noise == ROVER_OBS_POST_NOISE_UNIFORM) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (in & (1u << j)) v[j] = __fadd_rn(__fadd_rn(v[j], __fmul_rn(unit_uniform(w[j]), S.b)), S.a);
            } else if (S.noise == ROVER_OBS_POST_NOISE_GAUSSIAN) {
                float e[4];
                box_muller(w[0], w[1], e[0], e[1]);
                box_muller(w[2], w[3], e[2], e[3]);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (in & (1u << j)) v[j] = __fadd_rn(__fadd_rn(v[j], S.a), __fmul_rn(S.b, e[j]));
            } else if (S.noise == ROVER_OBS_POST_NOISE_CONSTANT) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (in & (1u << j)) v[j] = __fadd_rn(v[j], S.a);
            }
            if (S.has_clip) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (in & (1u << j)) v[j] = tclamp(v[j], S.clip_lo, S.clip_hi);
            }
            if (S.scale != 1.0f) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (in & (1u << j)) v[j] = __fmul_rn(v[j], S.scale);
            }
        }
        if (vec) {
            v4f o;
            o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
            *reinterpret_cast<v4f *>(p) = o;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (mask & (1u << j)) p[j] = v[j];
        }
    }
}

int refuse(const char *why) { return rover_internal_fail(ROVER_ERR_INVALID, "rover_obs_post_apply: %s", why); }

}  // namespace

extern "C" {

size_t rover_obs_post_segment_bytes(void) { return sizeof(rover_obs_post_segment); }

int rover_obs_post_apply(const rover_obs_post_segment *seg, int32_t n_seg, float *rows, int32_t width, int64_t pitch_floats,
                         int32_t n, uint64_t seed, uint64_t env_id_offset, uint64_t counter, uint32_t tag, void *stream)
{
    if (!seg || !rows) return refuse("NULL argument");
    if (n <= 0) return refuse("n must be > 0");
    if (width <= 0 || width > ROVER_OBS_POST_MAX_WIDTH) return refuse("width must be in [1, 262144]");
    if (pitch_floats < (int64_t)width) return refuse("pitch_floats must be >= width");
    if (n_seg < 1 || n_seg > ROVER_OBS_POST_MAX_SEGMENTS) return refuse("n_seg must be in [1, 8]");
    if (tag & 0xFFFFu) return refuse("the low 16 bits of tag must be clear");
    if (reinterpret_cast<uintptr_t>(rows) & 3) return refuse("rows must be 4-byte aligned");
    PostArgs A;
    int c_min = width, c_max = 0, draws = 0;
    for (int s = 0; s < n_seg; ++s) {
        const rover_obs_post_segment &S = seg[s];
        if (S.col_lo >= S.col_hi) return refuse("empty segment");
        if (S.col_lo < 0 || S.col_hi > width) return refuse("segment leaves the row");
        for (int o = 0; o < s; ++o)
            if (S.col_lo < seg[o].col_hi && seg[o].col_lo < S.col_hi) return refuse("segments overlap");
        if (S.noise < ROVER_OBS_POST_NOISE_NONE || S.noise > ROVER_OBS_POST_NOISE_CONSTANT) return refuse("unknown noise kind");
        if (!std::isfinite(S.a) || !std::isfinite(S.b) || !std::isfinite(S.scale)) return refuse("a, b and scale must be finite");
        if (S.noise == ROVER_OBS_POST_NOISE_UNIFORM && S.b < 0.0f) return refuse("uniform noise needs span >= 0");
        if (S.noise == ROVER_OBS_POST_NOISE_GAUSSIAN && S.b < 0.0f) return refuse("gaussian noise needs std >= 0");
        if (S.has_clip) {
            if (!std::isfinite(S.clip_lo) || !std::isfinite(S.clip_hi)) return refuse("clip bounds must be finite");
            if (S.clip_lo > S.clip_hi) return refuse("clip_lo must be <= clip_hi");
        }
        draws |= S.noise == ROVER_OBS_POST_NOISE_UNIFORM || S.noise == ROVER_OBS_POST_NOISE_GAUSSIAN;
        c_min = S.col_lo < c_min ? S.col_lo : c_min;
        c_max = S.col_hi > c_max ? S.col_hi : c_max;
        A.seg[s] = S;
    }
    for (int s = n_seg; s < ROVER_OBS_POST_MAX_SEGMENTS; ++s) A.seg[s] = rover_obs_post_segment{0, 0, 0, 0.0f, 0.0f, 0, 0.0f, 0.0f, 1.0f};
    int dev;
    if (int rc = device_of(rows, &dev, true)) return rc;
    DeviceGuard guard(dev);
    A.rows = rows;
    A.pitch = (long long)pitch_floats;
    A.q0 = c_min / 4;
    A.nq = (c_max + 3) / 4 - A.q0;
    A.total = (unsigned long long)n * (unsigned long long)A.nq;
    A.id0 = env_id_offset;
    A.n_seg = n_seg;
    A.width = width;
    A.k0 = (uint32_t)seed; A.k1 = (uint32_t)(seed >> 32);
    A.c1 = (uint32_t)counter; A.c2 = (uint32_t)(counter >> 32);
    A.tag = tag;
    A.draws = draws;
    const unsigned long long blocks = (A.total + TT - 1) / TT;
    hipLaunchKernelGGL(obs_post_kernel, dim3((unsigned)(blocks < (unsigned long long)MAX_BLOCKS ? blocks : MAX_BLOCKS)), dim3(TT), 0,
                       static_cast<hipStream_t>(stream), A);
    return launched("obs_post_kernel launch: %s");
}

}  // extern "C"
