// td3_actor_tile.hpp -- the TD3 actor's forward on one 16-row tile as a device function, shared by the kernels that run the actor in
// front of an exploration epilogue (td3_collect_kernels.hip, td3_explore_kernels.hip, sac_collect_kernels.hip), the exploration noise
// draw they share and the check of the actor's shapes.
//
// The network part is the single-network kernel's (policy_kernels.hip, ref_network<true>): the same tile, the same per-wave tile
// assignment, the same k-ordered MFMA chains and the same split-K combine order, so the mean is bit-identical to
// rover_policy_forward on the same rows (tests/test_gpu_td3_collect.py pins the two together).  The text is restated here and not
// shared with policy_kernels.hip, which stays byte for byte what it was, so its kernels' registers, schedule and time cannot move
// (DESIGN 16).  The rows of a ring slot are already sanitised, so the LDS-DMA staging is kept as it is.  Everything here is
// force-inlined into its kernel: a kernel that includes this file compiles to what it was with the text in place.
#ifndef ROVER_TD3_ACTOR_TILE_HPP
#define ROVER_TD3_ACTOR_TILE_HPP

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/rover_policy.h"
#include "train_math.hpp"

namespace {

constexpr int TDC_THREADS = 512;  // 8 waves, two per SIMD (as the single-network kernel)
constexpr int TDC_WAVES = TDC_THREADS / 64;
constexpr int TDC_ROWS = 16;      // observation rows per workgroup = M of the MFMA tile
constexpr int TDC_MAXT = 6;       // row pitch of the split-K partials: 16 * TDC_MAXT + 4 (POL_MAXT of policy_kernels.hip)
constexpr int TDC_PF = 3;         // k groups of B fragments in flight in the ragged wave of layer 1
constexpr int OBS = 965, PROP = 4, ENC_OFF = 3;
// LDS carve of the reference architecture (rover_policy_forward computes the same numbers from the descriptor)
constexpr int TILE_FLOATS = TDC_ROWS * OBS;                               // 15440
constexpr int PPITCH = 16 * TDC_MAXT + 4;                                 // 100
constexpr int PART_FLOATS = TDC_WAVES * TDC_ROWS * PPITCH;                // 12800
constexpr int ACT_PITCH = 256 + 4;
constexpr size_t LDS_BYTES = sizeof(float) * ((size_t)TILE_FLOATS + PART_FLOATS + 2 * TDC_ROWS * ACT_PITCH);
constexpr uint32_t NOISE_TAG = 0x54443300u;   // "TD3\0": word 3 of the Philox counter of the exploration noise, | action pair

typedef float v4f __attribute__((ext_vector_type(4)));

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

template <int NT>
__device__ __forceinline__ void mfma_one_group(v4f (&acc)[NT], const float (&a)[4], const v4f (&b)[NT])
{
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < NT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[i][j], acc[i], 0, 0, 0);
}
// acc[i] += A[16 x k-range] x B[k-range x 16] for NT column tiles, k groups [g0, g1) of 16 inputs with PF groups of B fragments in
// flight; the last group of a layer whose K is no multiple of 16 is peeled off (policy_kernels.hip, mfma_groups)
template <int NT, int PF>
__device__ __forceinline__ void mfma_groups(v4f (&acc)[NT], const float *arow_ptr, int akq, int K, const v4f *Wt, size_t tile_stride,
                                            int g0, int g1, int G)
{
    if (g0 >= g1) return;
    const bool ragged = (K & 15) != 0 && g1 == G;
    const int g_main = ragged ? g1 - 1 : g1;
    const int n_full = ((g_main - g0) / PF) * PF, rem = (g_main - g0) - n_full;
    v4f bq[PF][NT];
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
        for (int i = 0; i < NT; ++i) bq[u][i] = Wt[i * tile_stride + (size_t)min(g0 + u, G - 1) * 64];
    const float *ap = arow_ptr + 16 * g0 + akq;
    for (int gb = g0; gb < g0 + n_full; gb += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            float a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = ap[16 * u + 4 * j];
            mfma_one_group<NT>(acc, a, bq[u]);
#pragma unroll
            for (int i = 0; i < NT; ++i) bq[u][i] = Wt[i * tile_stride + (size_t)min(gb + u + PF, G - 1) * 64];
            __builtin_amdgcn_sched_barrier(0);
        }
        ap += 16 * PF;
    }
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        if (u < rem) {
            float a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = ap[16 * u + 4 * j];
            mfma_one_group<NT>(acc, a, bq[u]);
        } else if (u == rem && ragged) {
            float a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 16 * g_main + 4 * j + akq;
                const float v = arow_ptr[min(k, K - 1)];
                a[j] = k < K ? v : 0.0f;
            }
            mfma_one_group<NT>(acc, a, bq[u]);
        }
    }
}

// the single-network kernel's register blocks (policy_kernels.hip: ref_load, ref_mfma, ref_store); fragments b[g * STRIDE + i], i < NT
template <int NT, int GC, int STRIDE>
__device__ __forceinline__ void ref_load(v4f (&b)[GC * STRIDE], const v4f *Wt, size_t tile_stride)
{
#pragma unroll
    for (int g = 0; g < GC; ++g)
#pragma unroll
        for (int i = 0; i < NT; ++i) b[g * STRIDE + i] = Wt[i * tile_stride + (size_t)g * 64];
}
template <int NT, int GC, int STRIDE>
__device__ __forceinline__ void ref_mfma(v4f (&acc)[NT], const float *arow_ptr, int akq, const v4f (&b)[GC * STRIDE])
{
    const float *ap = arow_ptr + akq;
#pragma unroll
    for (int g = 0; g < GC; ++g) {
        float a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = ap[16 * g + 4 * j];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < NT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[g * STRIDE + i][j], acc[i], 0, 0, 0);
    }
}
// epilogue of a full-K layer: tiles t0 + 8 i; LeakyReLU; into an LDS activation buffer
template <int NT>
__device__ __forceinline__ void ref_store(const v4f (&acc)[NT], const float (&bv)[NT], float *dst_act, int dst_pitch, int t0, int N,
                                          int rows, int arow, int akq, float slope)
{
    float *pd = dst_act + 4 * akq * dst_pitch + 16 * t0 + arow;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * akq + j < rows && 16 * (t0 + TDC_WAVES * i) + arow < N)
                pd[j * dst_pitch + 16 * TDC_WAVES * i] = leaky(acc[i][j] + bv[i], slope);
}

// what a lane of waves 0 .. 3 holds after the forward: action column c of tile row r
struct Td3ActorLane {
    int r, c, row;   // row = the call's row index (tile base + r)
    bool live;       // r < rows of this tile && c < N
    float y;         // the actor's output (no final activation); defined for every lane, meaningful where live
    size_t o;        // row * N + c
};

// One workgroup of TDC_THREADS lanes runs the actor on rows [16 blockIdx.x, 16 blockIdx.x + 16) of `obs` (n rows in all) with
// LDS_BYTES of dynamic LDS at `lds`.  Returns false (wave-uniform) in waves 4 .. 7, which hold no output; true in waves 0 .. 3 with
// `out` filled.  Workgroup b reads replica b % n_copies of the packed buffer.
__device__ __forceinline__ bool td3_actor_tile(const rover_policy_desc &d, const float *__restrict__ packed, int n_copies,
                                               unsigned copy_floats, const float *__restrict__ obs, int n, float *lds, Td3ActorLane &out)
{
    packed += (size_t)(blockIdx.x % (unsigned)n_copies) * copy_floats;
    float *tile = lds;
    float *part = tile + TILE_FLOATS;
    float *buf0 = part + PART_FLOATS;
    float *buf1 = buf0 + TDC_ROWS * ACT_PITCH;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * TDC_ROWS;
    const int rows = min(TDC_ROWS, n - row0);
    constexpr int G2 = 5, G3 = 4, G4 = 16, G5 = 10;          // k groups of layers 2 .. 5 (K = 80, 64, 256, 160)
    constexpr int pitch = ACT_PITCH;
    const float slope = d.leaky_slope;
    const int arow = lane & 15, akq = lane >> 4;
    auto Wof = [&](int li) { return reinterpret_cast<const v4f *>(packed + d.layers[li].w_off) + lane; };
    auto Bof = [&](int li) { return packed + d.layers[li].b_off; };

    // ---- observation rows -> LDS by LDS-DMA (no staging registers: the rows of a ring slot are already sanitised), and, queued
    // right behind the copy, layer 1's weights.  Waves 0 .. 6 request 6 of their 8 k groups x 5 column tiles (30 fragments) in front
    // of the barrier, so the wait there is a counted vmcnt(30): the copy, not the weights.  Wave 7 holds the ragged end (k groups
    // 56 .. 60, the last one a single input) and takes the generic queue.
    constexpr int G1 = 61, GW1 = 8, T1 = 5, GA1 = 6, GB1 = GW1 - GA1;
    v4f f1a[GA1 * T1], f1b[GB1 * T1];
    const bool full1 = wave < 7;
    {
        const float *src = obs + (size_t)row0 * OBS;
        const int total = rows * OBS, total_pad = TDC_ROWS * OBS;
        const bool dma = rows == TDC_ROWS && (total & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
        if (dma) {
            const v4f *s4 = reinterpret_cast<const v4f *>(src);
            v4f *t4 = reinterpret_cast<v4f *>(tile);
            constexpr int n4 = TDC_ROWS * OBS / 4;
            const int wave_base = __builtin_amdgcn_readfirstlane(tid & ~63);
#pragma unroll
            for (int i0 = 0; i0 < n4; i0 += TDC_THREADS)
                if (i0 + tid < n4)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(s4 + i0 + tid),
                                                     (__attribute__((address_space(3))) void *)(t4 + i0 + wave_base), 16, 0, 0);
        } else {
            for (int i = tid; i < total_pad; i += TDC_THREADS) tile[i] = i < total ? src[i] : 0.0f;
        }
        asm volatile("" ::: "memory");   // the weight loads below stay BEHIND the copy in issue order (the counted wait relies on it)
        if (full1) ref_load<T1, GA1, T1>(f1a, Wof(0) + (size_t)(wave * GW1) * 64, (size_t)G1 * 64);
        if (full1) asm volatile("s_waitcnt vmcnt(30)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();   // the tile is complete

    v4f f2[G2];
    float bv2 = 0.0f;
    const bool has2 = wave < 4;
    // ---- layer 1: 961 -> 80, split-K, into buf0: accumulate (specialised for waves 0 .. 6), then the combine
    {
        const float *a1 = tile + ENC_OFF + arow * OBS;
        const int N1 = d.layers[0].N;
        v4f acc[T1];
#pragma unroll
        for (int i = 0; i < T1; ++i) acc[i] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
        if (full1) {
            ref_load<T1, GB1, T1>(f1b, Wof(0) + (size_t)(wave * GW1 + GA1) * 64, (size_t)G1 * 64);
            ref_mfma<T1, GA1, T1>(acc, a1 + 16 * (wave * GW1), akq, f1a);
            ref_mfma<T1, GB1, T1>(acc, a1 + 16 * (wave * GW1 + GA1), akq, f1b);
        } else mfma_groups<T1, TDC_PF>(acc, a1, akq, d.layers[0].K, Wof(0), (size_t)G1 * 64, 7 * GW1, G1, G1);
        float *pw = part + (wave * TDC_ROWS + 4 * akq) * PPITCH + arow;
#pragma unroll
        for (int i = 0; i < T1; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) pw[j * PPITCH + 16 * i] = acc[i][j];
        // layer 2's fragments (column tile `wave` of 4; waves 4 .. 7 have none) travel under layer 1's combine
        if (has2) {
            ref_load<1, G2, 1>(f2, Wof(1) + (size_t)wave * G2 * 64, 0);
            bv2 = Bof(1)[min(16 * wave + arow, d.layers[1].N - 1)];
        }
        // combine: ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), bias, LeakyReLU; thread -> (row, column), the column fastest
        constexpr int ncols = 16 * T1;
        const float inv = 1.0f / (float)ncols;
        const float *bias = Bof(0);
        __syncthreads();
        for (int e = tid; e < TDC_ROWS * ncols; e += TDC_THREADS) {
            const int r = (int)(((float)e + 0.5f) * inv), c = e - r * ncols;   // e / ncols, exact here
            float q[TDC_WAVES];
#pragma unroll
            for (int w = 0; w < TDC_WAVES; ++w) q[w] = part[(w * TDC_ROWS + r) * PPITCH + c];
            const float sum = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
            if (r < rows && c < N1) buf0[r * pitch + c] = leaky(sum + bias[c], slope);
        }
    }
    // layer 3's fragments (tiles wave, wave + 8 of 16) travel under layer 2
    v4f f3[G3 * 2];
    float bv3[2];
    ref_load<2, G3, 2>(f3, Wof(2) + (size_t)wave * G3 * 64, (size_t)TDC_WAVES * G3 * 64);
#pragma unroll
    for (int i = 0; i < 2; ++i) bv3[i] = Bof(2)[16 * (wave + TDC_WAVES * i) + arow];
    __syncthreads();   // buf0 = layer 1's activations

    // ---- layer 2: 80 -> 60 into buf1[:, 4 ..], proprioceptive columns in front (models.py:93-96)
    if (has2) {
        v4f acc[1] = {(v4f){0.0f, 0.0f, 0.0f, 0.0f}};
        ref_mfma<1, G2, 1>(acc, buf0 + arow * pitch, akq, f2);
        const float bv[1] = {bv2};
        ref_store<1>(acc, bv, buf1 + PROP, pitch, wave, d.layers[1].N, rows, arow, akq, slope);
    }
    if (tid < TDC_ROWS * PROP) buf1[(tid >> 2) * pitch + (tid & 3)] = tile[(tid >> 2) * OBS + (tid & 3)];
    // layer 4's fragments (tiles wave, wave + 8 of 10: two for waves 0 and 1, one otherwise) travel under layer 3
    v4f f4[G4 * 2];
    float bv4[2];
    const bool two4 = wave < 2;
    if (two4) ref_load<2, G4, 2>(f4, Wof(3) + (size_t)wave * G4 * 64, (size_t)TDC_WAVES * G4 * 64);
    else ref_load<1, G4, 2>(f4, Wof(3) + (size_t)wave * G4 * 64, 0);
    bv4[0] = Bof(3)[16 * wave + arow];
    bv4[1] = Bof(3)[min(16 * (wave + TDC_WAVES) + arow, d.layers[3].N - 1)];
    __syncthreads();   // buf1 = MLP input

    // ---- layer 3: 64 -> 256 into buf0
    {
        v4f acc[2] = {(v4f){0.0f, 0.0f, 0.0f, 0.0f}, (v4f){0.0f, 0.0f, 0.0f, 0.0f}};
        ref_mfma<2, G3, 2>(acc, buf1 + arow * pitch, akq, f3);
        ref_store<2>(acc, bv3, buf0, pitch, wave, d.layers[2].N, rows, arow, akq, slope);
    }
    // layer 5's fragments (tile `wave` of 8) travel under layer 4
    v4f f5[G5];
    ref_load<1, G5, 1>(f5, Wof(4) + (size_t)wave * G5 * 64, 0);
    const float bv5 = Bof(4)[16 * wave + arow];
    __syncthreads();   // buf0 = layer 3's activations

    // ---- layer 4: 256 -> 160 into buf1
    if (two4) {
        v4f acc[2] = {(v4f){0.0f, 0.0f, 0.0f, 0.0f}, (v4f){0.0f, 0.0f, 0.0f, 0.0f}};
        ref_mfma<2, G4, 2>(acc, buf0 + arow * pitch, akq, f4);
        ref_store<2>(acc, bv4, buf1, pitch, wave, d.layers[3].N, rows, arow, akq, slope);
    } else {
        v4f acc[1] = {(v4f){0.0f, 0.0f, 0.0f, 0.0f}};
        ref_mfma<1, G4, 2>(acc, buf0 + arow * pitch, akq, f4);
        const float bv[1] = {bv4[0]};
        ref_store<1>(acc, bv, buf1, pitch, wave, d.layers[3].N, rows, arow, akq, slope);
    }
    // layer 6's fragment (split-K: k group `wave` of 8, the one column tile) travels under layer 5
    const v4f f6 = Wof(5)[(size_t)wave * 64];
    __syncthreads();   // buf1 = layer 4's activations

    // ---- layer 5: 160 -> 128 into buf0
    {
        v4f acc[1] = {(v4f){0.0f, 0.0f, 0.0f, 0.0f}};
        ref_mfma<1, G5, 1>(acc, buf1 + arow * pitch, akq, f5);
        const float bv[1] = {bv5};
        ref_store<1>(acc, bv, buf0, pitch, wave, d.layers[4].N, rows, arow, akq, slope);
    }
    __syncthreads();   // buf0 = layer 5's activations

    // ---- layer 6: 128 -> out, split-K with one k group per wave, partials through `part`, the fixed combine order
    const int N = d.layers[5].N;
    {
        v4f acc = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
        const float *ap = buf0 + arow * pitch + 16 * wave + akq;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[4 * j], f6[j], acc, 0, 0, 0);
        float *pw = part + (wave * TDC_ROWS + 4 * akq) * PPITCH + arow;
#pragma unroll
        for (int j = 0; j < 4; ++j) pw[j * PPITCH] = acc[j];
    }
    __syncthreads();
    if (wave >= 4) return false;   // wave-uniform: the 16 x 16 sums live in waves 0 .. 3, lane (r, c) owns action column c of row r
    const int r = tid >> 4, c = tid & 15;
    float q[TDC_WAVES];
#pragma unroll
    for (int w = 0; w < TDC_WAVES; ++w) q[w] = part[(w * TDC_ROWS + r) * PPITCH + c];
    const float sum = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    out.r = r; out.c = c; out.row = row0 + r;
    out.live = r < rows && c < N;
    out.y = sum + Bof(5)[min(c, N - 1)];   // the actor's output (no final activation)
    out.o = (size_t)(row0 + r) * N + c;
    return true;
}

// The standard normal of (global env id g, counter, action column c): column c takes the cosine (even c) or sine (odd c) branch of
// pair c / 2 (rover_td3_collect.h; the uniforms, the Box-Muller form and sincospif of rover_rollout.h)
__device__ __forceinline__ float td3_noise_eps(uint32_t g, uint32_t ctr_lo, uint32_t ctr_hi, uint32_t tag, int c, uint32_t seed_lo,
                                               uint32_t seed_hi)
{
    uint32_t w4[4];
    philox4x32(g, ctr_lo, ctr_hi, tag | (uint32_t)(c >> 1), seed_lo, seed_hi, w4);
    float e0, e1;
    box_muller(w4[0], w4[1], e0, e1);
    return (c & 1) ? e1 : e0;
}

// mean + (noise * scale), clamped as torch.clamp: two fp32 operations, then a NaN sum stays NaN (fmaxf alone would make it `low`)
__device__ __forceinline__ float td3_add_noise_clamp(float mean, float noise, float scale, float low, float high)
{
    noise = noise * scale;
    const float a = mean + noise;
    const float cl = fminf(fmaxf(a, low), high);
    return a != a ? a : cl;
}

// the shapes the act kernels are written for (rover_policy_default_desc) with 1 .. 16 outputs under `final_act`
inline bool is_reference_actor(const rover_policy_desc *d, int final_act)
{
    if (d->obs_dim != OBS || d->prop_dim != PROP || d->enc_offset != ENC_OFF || d->enc_dim != 961 || d->n_enc != 2 || d->n_mlp != 4) return false;
    const int K[6] = {961, 80, 64, 256, 160, 128}, N[5] = {80, 60, 256, 160, 128};
    for (int i = 0; i < 6; ++i) {
        if (d->layers[i].K != K[i]) return false;
        if (i < 5 && (d->layers[i].N != N[i] || d->layers[i].act != ROVER_ACT_LEAKY_RELU)) return false;
        if ((d->layers[i].split_k != 0) != (i == 0 || i == 5)) return false;
    }
    return d->layers[5].N >= 1 && d->layers[5].N <= 16 && d->layers[5].act == final_act;
}

}  // namespace

#endif /* ROVER_TD3_ACTOR_TILE_HPP */
