// td3_collect_kernels.hip -- the off-policy half of an env step in two launches (gfx950 / CDNA4, wave64): before env.step the actor
// on a ring slot of the replay memory, counter-based exploration noise and the clamp; after it the env's raw rows sanitised into the
// next ring slot, reward / terminated / ring_pos of the transition and the batch's row indices.  See include/rover_td3_collect.h
// for the contract.
//
// The network part is the single-network kernel's (policy_kernels.hip, ref_network<true>): the same tile, the same per-wave tile
// assignment, the same k-ordered MFMA chains and the same split-K combine order, so the mean is bit-identical to
// rover_policy_forward on the same rows (tests/test_gpu_td3_collect.py pins the two together).  The text is restated here and not
// shared: policy_kernels.hip stays byte for byte what it was, so its kernels' registers, schedule and time cannot move.
// The rows of a ring slot are already sanitised, so the LDS-DMA staging is kept as it is.  One thing differs: the epilogue.  The
// 16 x 16 lanes of waves 0 .. 3 that hold the final-layer sums go on to the draw, the noise and the clamp.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_hip.h"
#include "../../include/rover_td3_collect.h"
#include "rover_internal.hpp"

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
constexpr uint32_t INDEX_TAG = 0x54335300u;   // "T3S\0": ... of the batch's row indices
constexpr int REC_THREADS = 256, REC_PER = 4; // record kernel: pieces (16 bytes, or one float on the scalar path) per thread

typedef float v4f __attribute__((ext_vector_type(4)));

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.0f ? v : v * slope; }

// torch.nan_to_num(x, nan = 0, posinf = FLT_MAX, neginf = 0): finite values (and -0) pass unchanged (rollout_kernels.hip)
__device__ __forceinline__ float sanitise(float x)
{
    if (x != x) return 0.0f;
    if (x == INFINITY) return FLT_MAX;
    if (x == -INFINITY) return 0.0f;
    return x;
}

// Philox4x32-10 (the text of rover_kernels.hip)
__device__ __forceinline__ void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct TdcLaunch {
    int n_copies;              // replicas of the packed buffer; workgroup b reads replica b % n_copies
    unsigned copy_floats;
    rover_td3_collect_hparams hp;
    uint32_t ctr_lo, ctr_hi;
    float *mean_out, *act_out, *env_act_out, *eps_out;
};

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

__global__ __launch_bounds__(TDC_THREADS) void rover_td3_collect_act_kernel(rover_policy_desc d, TdcLaunch L,
                                                                            const float *__restrict__ packed,
                                                                            const float *__restrict__ obs, int n)
{
    extern __shared__ __align__(16) float lds[];
    packed += (size_t)(blockIdx.x % (unsigned)L.n_copies) * L.copy_floats;
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
    if (wave >= 4) return;   // wave-uniform: the 16 x 16 sums live in waves 0 .. 3, lane (r, c) owns action column c of row r
    const int r = tid >> 4, c = tid & 15;
    float q[TDC_WAVES];
#pragma unroll
    for (int w = 0; w < TDC_WAVES; ++w) q[w] = part[(w * TDC_ROWS + r) * PPITCH + c];
    const float sum = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    const bool live = r < rows && c < N;
    const float y = sum + Bof(5)[min(c, N - 1)];   // the actor's output (no final activation)
    const size_t o = (size_t)(row0 + r) * N + c;
    if (live && L.mean_out) L.mean_out[o] = y;

    // ---- exploration epilogue (td3.explore): noise_std * eps, * scale, + mean as three separate operations, then the clamp (a NaN
    // sum stays NaN, as under torch.clamp)
    float a = y;
    if (L.hp.explore) {
        uint32_t w4[4];
        philox4x32((uint32_t)L.hp.env_id_offset + (uint32_t)(row0 + r), L.ctr_lo, L.ctr_hi, NOISE_TAG | (uint32_t)(c >> 1), L.hp.seed_lo, L.hp.seed_hi, w4);
        const float u1 = ((float)(w4[0] >> 9) + 0.5f) * 0x1p-23f, u2 = ((float)(w4[1] >> 9) + 0.5f) * 0x1p-23f;   // exact, inside (0, 1)
        const float rho = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincospif(2.0f * u2, &sn, &cs);             // the angle 2 pi u2 with an exact argument
        const float eps = (c & 1) ? rho * sn : rho * cs;
        float noise = L.hp.noise_std * eps;
        noise = noise * L.hp.noise_scale;
        a = y + noise;
        const float cl = fminf(fmaxf(a, L.hp.action_low), L.hp.action_high);
        a = a != a ? a : cl;                        // torch.clamp keeps a NaN; fmaxf alone would turn it into action_low
        if (live && L.eps_out) L.eps_out[o] = eps;
    }
    if (live) {
        L.act_out[o] = a;
        L.env_act_out[o] = a;
    }
}

struct RecLaunch {
    const float *rew;
    const uint8_t *terminated;
    float *rew_out;
    uint8_t *term_out;
    int32_t *ring_pos_entry;
    int32_t ring_pos_value;
    int64_t *idx_out;
    int batch;
    uint64_t mem_rows;
    uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi;
};

// VEC: both row pointers are 16-byte aligned.  Block b takes pieces [b * 1024, b * 1024 + 1024), thread t pieces t, t + 256, ...;
// the grid also covers n and batch threads for the record and the indices (blocks past the rows only do those).
template <bool VEC>
__global__ __launch_bounds__(REC_THREADS) void rover_td3_collect_record_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                                               size_t total, int n, RecLaunch R)
{
    const size_t gid = (size_t)blockIdx.x * REC_THREADS + threadIdx.x;
    const size_t base = (size_t)blockIdx.x * (REC_THREADS * REC_PER) + threadIdx.x;
    if (VEC) {
        const v4f *s4 = reinterpret_cast<const v4f *>(src);
        v4f *d4 = reinterpret_cast<v4f *>(dst);
        const size_t n4 = total >> 2;               // >= 241: a row is 965 floats
        if (base < n4) {
            v4f v[REC_PER];
#pragma unroll
            for (int u = 0; u < REC_PER; ++u) v[u] = __builtin_nontemporal_load(s4 + min(base + (size_t)u * REC_THREADS, n4 - 1));   // read once
#pragma unroll
            for (int u = 0; u < REC_PER; ++u) {
                const size_t i = base + (size_t)u * REC_THREADS;
                v4f s;
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j] = sanitise(v[u][j]);
                if (i < n4) d4[i] = s;              // a plain store: the next act launch reads this slot
            }
        }
        if (gid < (total & 3)) dst[4 * n4 + gid] = sanitise(src[4 * n4 + gid]);   // the floats behind the last whole piece
    } else {
#pragma unroll
        for (int u = 0; u < REC_PER; ++u) {
            const size_t i = base + (size_t)u * REC_THREADS;
            if (i < total) dst[i] = sanitise(src[i]);
        }
    }
    if (R.rew_out && gid < (size_t)n) {
        R.rew_out[gid] = R.rew[gid];
        R.term_out[gid] = R.terminated[gid] != 0 ? 1 : 0;
    }
    if (R.ring_pos_entry && gid == 0) *R.ring_pos_entry = R.ring_pos_value;
    if (R.idx_out && gid < (size_t)R.batch) {
        uint32_t w4[4];
        philox4x32((uint32_t)(gid >> 2), R.ctr_lo, R.ctr_hi, INDEX_TAG, R.seed_lo, R.seed_hi, w4);
        const uint32_t w = w4[gid & 3];
        R.idx_out[gid] = (int64_t)(((uint64_t)w * R.mem_rows) >> 32);   // mem_rows <= 2^32: the product fits 64 bits
    }
}

// the shapes the act kernel is written for (rover_policy_default_desc), with no final activation
bool is_reference_actor(const rover_policy_desc *d)
{
    if (d->obs_dim != OBS || d->prop_dim != PROP || d->enc_offset != ENC_OFF || d->enc_dim != 961 || d->n_enc != 2 || d->n_mlp != 4) return false;
    const int K[6] = {961, 80, 64, 256, 160, 128}, N[5] = {80, 60, 256, 160, 128};
    for (int i = 0; i < 6; ++i) {
        if (d->layers[i].K != K[i]) return false;
        if (i < 5 && (d->layers[i].N != N[i] || d->layers[i].act != ROVER_ACT_LEAKY_RELU)) return false;
        if ((d->layers[i].split_k != 0) != (i == 0 || i == 5)) return false;
    }
    return d->layers[5].N >= 1 && d->layers[5].N <= 16 && d->layers[5].act == ROVER_ACT_NONE;
}

}  // namespace

extern "C" {

int rover_td3_collect_default_hparams(rover_td3_collect_hparams *h)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "hparams is NULL");
    memset(h, 0, sizeof(*h));
    h->seed_lo = 42u; h->seed_hi = 0u;
    h->env_id_offset = 0;
    h->explore = 0;
    h->noise_std = 0.0f; h->noise_scale = 1.0f;
    h->action_low = -1.0f; h->action_high = 1.0f;     // skrl TD3: the action space's bounds
    return ROVER_OK;
}

size_t rover_td3_collect_hparams_bytes(void) { return sizeof(rover_td3_collect_hparams); }

int rover_td3_collect_act(const rover_policy_desc *actor, const float *packed, int32_t n_copies, const rover_td3_collect_hparams *h,
                          uint64_t counter, const float *obs, int32_t n, float *mean_out, float *act_out, float *env_act_out,
                          float *eps_out, void *stream)
{
    if (!actor || !h) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_act: NULL descriptor / hparams");
    if (!packed || !obs || !act_out || !env_act_out) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_act: NULL required pointer");
    if (n < 1 || n_copies < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_act: n and n_copies must be >= 1");
    if (reinterpret_cast<uintptr_t>(packed) & 15) return rover_internal_fail(ROVER_ERR_INVALID, "packed weights must be 16-byte aligned");
    if (h->explore != 0 && h->explore != 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_act: explore must be 0 or 1");
    if (h->explore && !(h->action_low <= h->action_high))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_act: action_low > action_high");
    if (!is_reference_actor(actor))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "rover_td3_collect_act: the actor must have the reference architecture with no "
                                                          "final activation");
    TdcLaunch L;
    L.n_copies = n_copies;
    L.copy_floats = (unsigned)rover_policy_packed_floats(actor);
    L.hp = *h;
    L.ctr_lo = (uint32_t)(counter & 0xFFFFFFFFu);
    L.ctr_hi = (uint32_t)(counter >> 32);
    L.mean_out = mean_out; L.act_out = act_out; L.env_act_out = env_act_out; L.eps_out = eps_out;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(rover_td3_collect_act_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(rover_td3_collect_act_kernel, dim3(ceil_div(n, TDC_ROWS)), dim3(TDC_THREADS), LDS_BYTES,
                       static_cast<hipStream_t>(stream), *actor, L, packed, obs, n);
    e = hipGetLastError();
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "rover_td3_collect_act_kernel launch: %s", hipGetErrorString(e));
    return ROVER_OK;
}

int rover_td3_collect_record(const float *obs_raw, int32_t n, float *ring_slot_out, const float *rew, const uint8_t *terminated,
                             float *rew_out, uint8_t *term_out, int32_t *ring_pos_entry, int32_t ring_pos_value, int64_t *idx_out,
                             int32_t batch, int64_t mem_rows, const rover_td3_collect_hparams *h, uint64_t counter, void *stream)
{
    if (!obs_raw || !ring_slot_out) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: NULL rows");
    if (n < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: n must be >= 1");
    const size_t total = (size_t)n * OBS;
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(obs_raw), b = reinterpret_cast<uintptr_t>(ring_slot_out);
        if (a < b + total * sizeof(float) && b < a + total * sizeof(float))
            return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: ring_slot_out must not alias obs_raw");
    }
    const int given = (rew != nullptr) + (terminated != nullptr) + (rew_out != nullptr) + (term_out != nullptr);
    if (given != 0 && given != 4)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: rew, terminated, rew_out, term_out: all or none NULL");
    if (idx_out) {
        if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: hparams is NULL");
        if (batch < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: batch must be >= 1");
        if (mem_rows < 1 || mem_rows > ((int64_t)1 << 32))
            return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: mem_rows must lie in [1, 2^32]");
    }
    const bool vec = ((reinterpret_cast<uintptr_t>(obs_raw) | reinterpret_cast<uintptr_t>(ring_slot_out)) & 15) == 0;
    const size_t units = vec ? total >> 2 : total, per_block = (size_t)REC_THREADS * REC_PER;
    size_t blocks = (units + per_block - 1) / per_block;
    const size_t threads = (size_t)(idx_out && batch > n ? batch : n);
    if (blocks < (threads + REC_THREADS - 1) / REC_THREADS) blocks = (threads + REC_THREADS - 1) / REC_THREADS;
    if (blocks > 0x7FFFFFFFu) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: n too large");
    RecLaunch R;
    R.rew = rew; R.terminated = terminated; R.rew_out = rew_out; R.term_out = term_out;
    R.ring_pos_entry = ring_pos_entry; R.ring_pos_value = ring_pos_value;
    R.idx_out = idx_out; R.batch = idx_out ? batch : 0; R.mem_rows = idx_out ? (uint64_t)mem_rows : 1u;
    R.seed_lo = h ? h->seed_lo : 0u; R.seed_hi = h ? h->seed_hi : 0u;
    R.ctr_lo = (uint32_t)(counter & 0xFFFFFFFFu);
    R.ctr_hi = (uint32_t)(counter >> 32);
    if (vec)
        hipLaunchKernelGGL(rover_td3_collect_record_kernel<true>, dim3((unsigned)blocks), dim3(REC_THREADS), 0,
                           static_cast<hipStream_t>(stream), obs_raw, ring_slot_out, total, n, R);
    else
        hipLaunchKernelGGL(rover_td3_collect_record_kernel<false>, dim3((unsigned)blocks), dim3(REC_THREADS), 0,
                           static_cast<hipStream_t>(stream), obs_raw, ring_slot_out, total, n, R);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "rover_td3_collect_record_kernel launch: %s", hipGetErrorString(e));
    return ROVER_OK;
}

}  // extern "C"
