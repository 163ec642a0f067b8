// rollout_kernels.hip -- the on-policy rollout step in one launch (gfx950 / CDNA4, wave64): sanitise the env's raw observation rows
// into the rollout buffer, run the actor and the critic on the staged tile, draw counter-based Gaussian actions, clip them for the
// env and evaluate the log-probability.  See include/rover_rollout.h for the contract.
//
// The network part is the pair kernel's (policy_kernels.hip, ref_pair_network): the same tile, the same per-wave tile assignment,
// the same k-ordered MFMA chains and the same split-K combine order, so mean and value are bit-identical to
// rover_policy_forward_pair on the sanitised rows (tests/test_gpu_rollout.py pins the two together).  The text is restated here
// and not shared: policy_kernels.hip stays byte for byte what it was, so the pair kernel's registers, schedule and time cannot
// move (DESIGN 11 records what a code move cost the camera kernel).  Two things differ from the pair kernel:
//   * staging: the rows pass through registers (the pair kernel's LDS-DMA cannot touch the values), every element goes through
//     nan_to_num(nan = 0, posinf = FLT_MAX, neginf = 0), and the sanitised rows are also stored to the rollout buffer;
//   * epilogue: the 16 x 16 lanes that hold the actor's final-layer sums go on to the draws, the actions and the log-probability.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/rover_hip.h"
#include "../../include/rover_rollout.h"
#include "rover_internal.hpp"
#include "train_math.hpp"

namespace {

constexpr int ROL_THREADS = 512;  // 8 waves, two per SIMD (as the pair kernel)
constexpr int ROL_WAVES = ROL_THREADS / 64;
constexpr int ROL_ROWS = 16;      // observation rows per workgroup = M of the MFMA tile
constexpr int ROL_PF = 3;         // k groups of B fragments in flight in the ragged wave of layer 1
constexpr int OBS = 965, PROP = 4, ENC_OFF = 3;
// LDS carve of the reference architecture (rover_policy_forward_pair computes the same numbers from the descriptor)
constexpr int TILE_FLOATS = ROL_ROWS * OBS;                       // 15440
constexpr int PART_FLOATS = ROL_WAVES * ROL_ROWS * (16 * 6 + 4);  // 12800
constexpr int ACT_PITCH = 256 + 4;
constexpr size_t LDS_BYTES = sizeof(float) * ((size_t)TILE_FLOATS + PART_FLOATS + 2 * ROL_ROWS * ACT_PITCH);
constexpr uint32_t ROL_TAG = 0x524F4C00u;   // "ROL\0": word 3 of the Philox counter, | action pair

typedef float v4f __attribute__((ext_vector_type(4)));

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

__device__ __forceinline__ float activate(float v, int act, float slope)
{
    if (act == ROVER_ACT_LEAKY_RELU) return v > 0.0f ? v : v * slope;
    if (act == ROVER_ACT_TANH) return rv_tanhf(v);
    return v;
}

struct RolLaunch {
    int n_copies;              // replicas of the packed buffers; workgroup b reads replica b % n_copies
    unsigned copy_floats_a, copy_floats_b;
    rover_rollout_hparams hp;
    uint32_t ctr_lo, ctr_hi;
    const float *log_std;
    float *obs_out, *mean_out, *val_out, *act_out, *env_act_out, *logp_out, *eps_out;
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

// the pair kernel's fragment queues (Wt[i]: the wave-uniform start of tile i's fragments)
template <int NT, int QD>
__device__ __forceinline__ void pq_preload(v4f (&q)[QD][NT], const v4f *const (&Wt)[NT], int lane)
{
#pragma unroll
    for (int u = 0; u < QD; ++u)
#pragma unroll
        for (int i = 0; i < NT; ++i) q[u][i] = Wt[i][u * 64 + lane];
}
template <int NT, int GC, int QD>
__device__ __forceinline__ void pq_run(v4f (&acc)[NT], const float *const (&ap)[NT], v4f (&q)[QD][NT], const v4f *const (&Wt)[NT], int lane)
{
    static_assert(QD <= GC, "queue deeper than the layer");
#pragma unroll
    for (int g = 0; g < GC; ++g) {
        const int slot = g % QD;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < NT; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[i][16 * g + 4 * j], q[slot][i][j], acc[i], 0, 0, 0);
        if (g + QD < GC) {
#pragma unroll
            for (int i = 0; i < NT; ++i) q[slot][i] = Wt[i][(g + QD) * 64 + lane];
        }
    }
}
__device__ __forceinline__ void pq_store(const v4f &acc, float bv, float *dst, int pitch, int tile, int N, int rows, int arow, int akq,
                                         float slope)
{
    float *pd = dst + 4 * akq * pitch + 16 * tile + arow;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * akq + j < rows && 16 * tile + arow < N) pd[j * pitch] = activate(acc[j] + bv, ROVER_ACT_LEAKY_RELU, slope);
}

// NT_STORE: the sanitised rows leave with a non-temporal store (the slot is read again by the update only)
template <bool NT_STORE>
__global__ __launch_bounds__(ROL_THREADS) void rover_rollout_act_kernel(rover_policy_desc da, rover_policy_desc db, RolLaunch L,
                                                                        const float *__restrict__ packed_a,
                                                                        const float *__restrict__ packed_b,
                                                                        const float *__restrict__ obs, int n)
{
    extern __shared__ __align__(16) float lds[];
    packed_a += (size_t)(blockIdx.x % (unsigned)L.n_copies) * L.copy_floats_a;
    packed_b += (size_t)(blockIdx.x % (unsigned)L.n_copies) * L.copy_floats_b;
    constexpr int G1 = 61, GW1 = 8, T1 = 5, G2 = 5, G3 = 4, G4 = 16, G5 = 10;
    constexpr int PP1 = 16 * T1 + 4;                         // row pitch of the layer-1 partials (five tiles)
    constexpr int PP6 = 20;                                  // ... of the layer-6 partials (one tile)
    constexpr int pitch = ACT_PITCH;
    float *tile = lds;
    float *partA = tile + TILE_FLOATS;
    float *bufA0 = partA + PART_FLOATS, *bufA1 = bufA0 + ROL_ROWS * pitch;
    float *partB = tile;                                     // the critic's share of the tile region (free after layer 1)
    float *bufB0 = tile + ROL_WAVES * ROL_ROWS * PP1, *bufB1 = tile;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * ROL_ROWS;
    const int rows = min(ROL_ROWS, n - row0);
    const float slope = da.leaky_slope;
    const int arow = lane & 15, akq = lane >> 4;
    auto Wof = [&](int net, int li) { return reinterpret_cast<const v4f *>((net ? packed_b : packed_a) + (net ? db : da).layers[li].w_off); };
    auto Bof = [&](int net, int li) { return (net ? packed_b : packed_a) + (net ? db : da).layers[li].b_off; };

    // ---- raw rows -> registers -> nan_to_num -> LDS tile (+ the rollout buffer); layer 1's first k group queued behind the loads
    constexpr int QD1 = 1;
    const bool full1 = wave < 7;
    v4f q1[QD1][2 * T1];
    const v4f *W1[2 * T1];
#pragma unroll
    for (int i = 0; i < 2 * T1; ++i) W1[i] = Wof(i >= T1, 0) + ((size_t)(i % T1) * G1 + (size_t)wave * GW1) * 64;
    {
        const float *src = obs + (size_t)row0 * OBS;
        float *dst = L.obs_out ? L.obs_out + (size_t)row0 * OBS : nullptr;
        const int total = rows * OBS, total_pad = ROL_ROWS * OBS;
        const bool vec = rows == ROL_ROWS && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
        if (vec) {   // a full tile is 3860 16-byte pieces: eight loads in flight per lane, the last trip partly masked
            const v4f *s4 = reinterpret_cast<const v4f *>(src);
            v4f *t4 = reinterpret_cast<v4f *>(tile), *d4 = reinterpret_cast<v4f *>(dst);
            constexpr int n4 = ROL_ROWS * OBS / 4;
            v4f r[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) r[u] = __builtin_nontemporal_load(s4 + min(tid + u * ROL_THREADS, n4 - 1));   // read once
            if (full1) pq_preload<2 * T1, QD1>(q1, W1, lane);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = tid + u * ROL_THREADS;
                v4f v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = sanitise(r[u][j]);
                if (i < n4) {
                    t4[i] = v;
                    if (dst) {
                        if (NT_STORE) __builtin_nontemporal_store(v, d4 + i);
                        else d4[i] = v;
                    }
                }
            }
        } else {
            for (int i = tid; i < total_pad; i += ROL_THREADS) {
                const float v = i < total ? sanitise(src[i]) : 0.0f;
                tile[i] = v;
                if (dst && i < total) dst[i] = v;
            }
            if (full1) pq_preload<2 * T1, QD1>(q1, W1, lane);
        }
    }
    __syncthreads();   // the tile is complete
    const float prop = tid < ROL_ROWS * PROP ? tile[(tid >> 2) * OBS + (tid & 3)] : 0.0f;   // models.py:93-96, saved before the tile is reused

    // ---- layer 1 of both networks: 961 -> 80, split-K over the waves
    v4f acc1[2 * T1];
#pragma unroll
    for (int i = 0; i < 2 * T1; ++i) acc1[i] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    {
        const float *a1 = tile + ENC_OFF + arow * OBS;
        if (full1) {
            const float *ap[2 * T1];
#pragma unroll
            for (int i = 0; i < 2 * T1; ++i) ap[i] = a1 + 16 * (wave * GW1) + akq;
            pq_run<2 * T1, GW1, QD1>(acc1, ap, q1, W1, lane);
        } else {   // the ragged end (k groups 56 .. 60, the last one a single input), one network after the other
            v4f accA[T1], accB[T1];
#pragma unroll
            for (int i = 0; i < T1; ++i) { accA[i] = (v4f){0.0f, 0.0f, 0.0f, 0.0f}; accB[i] = (v4f){0.0f, 0.0f, 0.0f, 0.0f}; }
            mfma_groups<T1, ROL_PF>(accA, a1, akq, da.layers[0].K, Wof(0, 0) + lane, (size_t)G1 * 64, 7 * GW1, G1, G1);
            mfma_groups<T1, ROL_PF>(accB, a1, akq, db.layers[0].K, Wof(1, 0) + lane, (size_t)G1 * 64, 7 * GW1, G1, G1);
#pragma unroll
            for (int i = 0; i < T1; ++i) { acc1[i] = accA[i]; acc1[T1 + i] = accB[i]; }
        }
    }
    // layer 2's fragments (waves 0 .. 3 the actor's four column tiles, 4 .. 7 the critic's) travel under the combine
    const int net2 = wave >> 2, t2 = wave & 3;
    v4f q2[G2][1];
    const v4f *W2[1] = {Wof(net2, 1) + (size_t)t2 * G2 * 64};
    pq_preload<1, G2>(q2, W2, lane);
    const float bv2 = Bof(net2, 1)[min(16 * t2 + arow, da.layers[1].N - 1)];
    __syncthreads();   // every wave has read its layer-1 A fragments: the tile region is free
    {
        float *pa = partA + (wave * ROL_ROWS + 4 * akq) * PP1 + arow, *pb = partB + (wave * ROL_ROWS + 4 * akq) * PP1 + arow;
#pragma unroll
        for (int i = 0; i < T1; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) { pa[j * PP1 + 16 * i] = acc1[i][j]; pb[j * PP1 + 16 * i] = acc1[T1 + i][j]; }
    }
    __syncthreads();
    {   // combine: ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), bias, LeakyReLU; 16 x 80 outputs per network
        const int N1 = da.layers[0].N;
        const float *b1a = Bof(0, 0), *b1b = Bof(1, 0);
        for (int e = tid; e < 2 * ROL_ROWS * 16 * T1; e += ROL_THREADS) {
            const int net = e >= ROL_ROWS * 16 * T1, ee = e - net * ROL_ROWS * 16 * T1;
            const int r = (int)(((float)ee + 0.5f) * (1.0f / (float)(16 * T1))), c = ee - r * 16 * T1;
            const float *pp = (net ? partB : partA) + r * PP1 + c;
            float qq[ROL_WAVES];
#pragma unroll
            for (int w = 0; w < ROL_WAVES; ++w) qq[w] = pp[w * ROL_ROWS * PP1];
            const float sum = ((qq[0] + qq[1]) + (qq[2] + qq[3])) + ((qq[4] + qq[5]) + (qq[6] + qq[7]));
            if (r < rows && c < N1) (net ? bufB0 : bufA0)[r * pitch + c] = activate(sum + (net ? b1b : b1a)[c], ROVER_ACT_LEAKY_RELU, slope);
        }
    }
    // layer 3's fragments: tiles tt = wave + 8 i of 32 (tt < 16: actor tile tt, else critic tile tt - 16)
    v4f q3[G3][4];
    const v4f *W3[4];
    float bv3[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int tt = wave + ROL_WAVES * i, net = tt >> 4, t = tt & 15;
        W3[i] = Wof(net, 2) + (size_t)t * G3 * 64;
        bv3[i] = Bof(net, 2)[16 * t + arow];
    }
    pq_preload<4, G3>(q3, W3, lane);
    __syncthreads();   // bufA0 / bufB0 = layer 1's activations; partB is dead (bufB1 overlays it)

    // ---- layer 2: 80 -> 60 into buf?1[:, 4 ..], the proprioceptive columns in front
    {
        v4f acc[1] = {(v4f){0.0f, 0.0f, 0.0f, 0.0f}};
        const float *ap[1] = {(net2 ? bufB0 : bufA0) + arow * pitch + akq};
        pq_run<1, G2, G2>(acc, ap, q2, W2, lane);
        pq_store(acc[0], bv2, (net2 ? bufB1 : bufA1) + PROP, pitch, t2, da.layers[1].N, rows, arow, akq, slope);
    }
    if (tid < ROL_ROWS * PROP) {
        bufA1[(tid >> 2) * pitch + (tid & 3)] = prop;
        bufB1[(tid >> 2) * pitch + (tid & 3)] = prop;
    }
    // layer 4's fragments: twenty tiles, tt = wave + 8 i: three for waves 0 .. 3, two for waves 4 .. 7; the first four k groups
    constexpr int QD4 = 4;
    const bool three4 = wave < 4;
    v4f q4[QD4][3];
    const v4f *W4[3];
    float bv4[3];
    int net4[3], t4[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int tt = min(wave + ROL_WAVES * i, 19);
        net4[i] = tt >= 10; t4[i] = tt - 10 * net4[i];
        W4[i] = Wof(net4[i], 3) + (size_t)t4[i] * G4 * 64;
        bv4[i] = Bof(net4[i], 3)[16 * t4[i] + arow];
    }
    if (three4) {
        pq_preload<3, QD4>(q4, W4, lane);
    } else {
        v4f q42[QD4][2];
        const v4f *W42[2] = {W4[0], W4[1]};
        pq_preload<2, QD4>(q42, W42, lane);
#pragma unroll
        for (int u = 0; u < QD4; ++u) { q4[u][0] = q42[u][0]; q4[u][1] = q42[u][1]; }
    }
    __syncthreads();   // buf?1 = the MLP inputs

    // ---- layer 3: 64 -> 256 into buf?0
    {
        v4f acc[4];
        const float *ap[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[i] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
            ap[i] = (i >= 2 ? bufB1 : bufA1) + arow * pitch + akq;      // tt = wave + 8 i: i < 2 actor, else critic
        }
        pq_run<4, G3, G3>(acc, ap, q3, W3, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            pq_store(acc[i], bv3[i], i >= 2 ? bufB0 : bufA0, pitch, (wave + ROL_WAVES * i) & 15, da.layers[2].N, rows, arow, akq, slope);
    }
    // layer 5's fragments: actor tile `wave`, critic tile `wave`; the first three of ten k groups
    constexpr int QD5 = 3;
    v4f q5[QD5][2];
    const v4f *W5[2] = {Wof(0, 4) + (size_t)wave * G5 * 64, Wof(1, 4) + (size_t)wave * G5 * 64};
    const float bv5[2] = {Bof(0, 4)[16 * wave + arow], Bof(1, 4)[16 * wave + arow]};
    pq_preload<2, QD5>(q5, W5, lane);
    __syncthreads();   // buf?0 = layer 3's activations

    // ---- layer 4: 256 -> 160 into buf?1
    if (three4) {
        v4f acc[3];
        const float *ap[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            acc[i] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
            ap[i] = (net4[i] ? bufB0 : bufA0) + arow * pitch + akq;
        }
        pq_run<3, G4, QD4>(acc, ap, q4, W4, lane);
#pragma unroll
        for (int i = 0; i < 3; ++i) pq_store(acc[i], bv4[i], net4[i] ? bufB1 : bufA1, pitch, t4[i], da.layers[3].N, rows, arow, akq, slope);
    } else {
        v4f acc[2];
        const float *ap[2];
        v4f q42[QD4][2];
        const v4f *W42[2] = {W4[0], W4[1]};
#pragma unroll
        for (int u = 0; u < QD4; ++u) { q42[u][0] = q4[u][0]; q42[u][1] = q4[u][1]; }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            acc[i] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
            ap[i] = (net4[i] ? bufB0 : bufA0) + arow * pitch + akq;
        }
        pq_run<2, G4, QD4>(acc, ap, q42, W42, lane);
#pragma unroll
        for (int i = 0; i < 2; ++i) pq_store(acc[i], bv4[i], net4[i] ? bufB1 : bufA1, pitch, t4[i], da.layers[3].N, rows, arow, akq, slope);
    }
    // layer 6's fragments (split-K: k group `wave` of 8, the one column tile of each network) travel under layer 5
    const v4f f6a = Wof(0, 5)[wave * 64 + lane], f6b = Wof(1, 5)[wave * 64 + lane];
    __syncthreads();   // buf?1 = layer 4's activations

    // ---- layer 5: 160 -> 128 into buf?0
    {
        v4f acc[2] = {(v4f){0.0f, 0.0f, 0.0f, 0.0f}, (v4f){0.0f, 0.0f, 0.0f, 0.0f}};
        const float *ap[2] = {bufA1 + arow * pitch + akq, bufB1 + arow * pitch + akq};
        pq_run<2, G5, QD5>(acc, ap, q5, W5, lane);
        pq_store(acc[0], bv5[0], bufA0, pitch, wave, da.layers[4].N, rows, arow, akq, slope);
        pq_store(acc[1], bv5[1], bufB0, pitch, wave, db.layers[4].N, rows, arow, akq, slope);
    }
    __syncthreads();   // buf?0 = layer 5's activations

    // ---- layer 6: 128 -> out, split-K with one k group per wave, both networks; partials through partA ([0, 2560) actor, then critic)
    v4f acA = (v4f){0.0f, 0.0f, 0.0f, 0.0f}, acB = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    const float *apA = bufA0 + arow * pitch + 16 * wave + akq, *apB = bufB0 + arow * pitch + 16 * wave + akq;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acA = __builtin_amdgcn_mfma_f32_16x16x4f32(apA[4 * j], f6a[j], acA, 0, 0, 0);
        acB = __builtin_amdgcn_mfma_f32_16x16x4f32(apB[4 * j], f6b[j], acB, 0, 0, 0);
    }
    float *pw = partA + (wave * ROL_ROWS + 4 * akq) * PP6 + arow;
#pragma unroll
    for (int j = 0; j < 4; ++j) { pw[j * PP6] = acA[j]; pw[ROL_WAVES * ROL_ROWS * PP6 + j * PP6] = acB[j]; }
    __syncthreads();
    const int net = tid >> 8, e = tid & 255, r = e >> 4, c = e & 15;   // waves 0 .. 3: the actor's 16 x 16 sums, 4 .. 7: the critic's
    const rover_policy_desc &d = net ? db : da;
    const int N = d.layers[5].N;
    const float *pp = partA + net * ROL_WAVES * ROL_ROWS * PP6 + r * PP6 + c;
    float qq[ROL_WAVES];
#pragma unroll
    for (int w = 0; w < ROL_WAVES; ++w) qq[w] = pp[w * ROL_ROWS * PP6];
    const float sum = ((qq[0] + qq[1]) + (qq[2] + qq[3])) + ((qq[4] + qq[5]) + (qq[6] + qq[7]));
    const bool live = r < rows && c < N;
    const float y = activate(sum + Bof(net, 5)[min(c, N - 1)], d.layers[5].act, d.leaky_slope);   // the policy mean / the value
    const size_t o = (size_t)(row0 + r) * N + c;
    if (live) (net ? L.val_out : L.mean_out)[o] = y;   // the value leaves from the lane that holds it: nothing crosses lanes for it

    // ---- sampling epilogue on the actor's lanes (waves 0 .. 3, wave-uniform): lane (r, c) owns action column c of row r
    const bool draw = L.act_out || L.env_act_out || L.logp_out || L.eps_out;
    if (!draw || wave >= 4) return;
    uint32_t w4[4];
    philox4x32((uint32_t)(L.hp.env_id_offset + row0 + r), L.ctr_lo, L.ctr_hi, ROL_TAG | (uint32_t)(c >> 1), L.hp.seed_lo, L.hp.seed_hi, w4);
    const float u1 = ((float)(w4[0] >> 9) + 0.5f) * 0x1p-23f, u2 = ((float)(w4[1] >> 9) + 0.5f) * 0x1p-23f;   // exact, inside (0, 1)
    const float rho = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);             // the angle 2 pi u2 with an exact argument
    const float eps = (c & 1) ? rho * sn : rho * cs;
    const float ls = fminf(fmaxf(L.log_std[min(c, N - 1)], L.hp.log_std_min), L.hp.log_std_max);
    const float sd = expf(ls);
    const float noise = sd * eps;
    const float a = y + noise;                  // a separate multiply and add
    const float ea = L.hp.clip_actions ? fminf(fmaxf(a, L.hp.action_low), L.hp.action_high) : a;
    const float x = (a - y) / sd;               // rover_ppo_minibatch forms x, and the row sum below, the same way
    const float term = -0.5f * x * x - ls - 0.9189385332f;
    float lp = __shfl(term, lane & ~15);        // column 0 first, then the others in order (all 64 lanes take part)
    for (int k = 1; k < N; ++k) lp = lp + __shfl(term, (lane & ~15) + k);
    if (live) {
        if (L.eps_out) L.eps_out[o] = eps;
        if (L.act_out) L.act_out[o] = a;
        if (L.env_act_out) L.env_act_out[o] = ea;
    }
    if (L.logp_out && c == 0 && r < rows) L.logp_out[row0 + r] = lp;
}

__global__ __launch_bounds__(256) void rover_rollout_record_kernel(const float *__restrict__ rew, const uint8_t *__restrict__ terminated,
                                                                   const uint8_t *__restrict__ truncated, int n,
                                                                   float *__restrict__ rew_out, float *__restrict__ done_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    rew_out[i] = rew[i];
    done_out[i] = (terminated[i] | truncated[i]) ? 1.0f : 0.0f;
}

// reward shaping and skrl's time-limit bootstrap in the record launch; every product and sum is formed (no contraction)
__global__ __launch_bounds__(256) void rover_rollout_record_shaped_kernel(const float *__restrict__ rew, const uint8_t *__restrict__ terminated,
                                                                          const uint8_t *__restrict__ truncated, const float *__restrict__ val,
                                                                          int n, float scale, float discount, int bootstrap,
                                                                          float *__restrict__ rew_out, float *__restrict__ done_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t tr = truncated[i];
    float r = __fmul_rn(rew[i], scale);
    if (bootstrap) r = __fadd_rn(r, __fmul_rn(__fmul_rn(discount, val[i]), tr ? 1.0f : 0.0f));
    rew_out[i] = r;
    done_out[i] = (terminated[i] | tr) ? 1.0f : 0.0f;
}

// the shapes the kernel is written for (rover_policy_default_desc)
bool is_reference_architecture(const rover_policy_desc *d)
{
    if (d->obs_dim != OBS || d->prop_dim != PROP || d->enc_offset != ENC_OFF || d->enc_dim != 961 || d->n_enc != 2 || d->n_mlp != 4) return false;
    const int K[6] = {961, 80, 64, 256, 160, 128}, N[5] = {80, 60, 256, 160, 128};
    for (int i = 0; i < 6; ++i) {
        if (d->layers[i].K != K[i]) return false;
        if (i < 5 && (d->layers[i].N != N[i] || d->layers[i].act != ROVER_ACT_LEAKY_RELU)) return false;
        if ((d->layers[i].split_k != 0) != (i == 0 || i == 5)) return false;
    }
    return d->layers[5].N >= 1 && d->layers[5].N <= 16;
}

}  // namespace

extern "C" {

int rover_rollout_default_hparams(rover_rollout_hparams *h)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "hparams is NULL");
    memset(h, 0, sizeof(*h));
    h->seed_lo = 42u; h->seed_hi = 0u;
    h->env_id_offset = 0;
    h->clip_actions = 1;
    h->action_low = -1.0f; h->action_high = 1.0f;     // models.py:66
    h->log_std_min = -20.0f; h->log_std_max = 2.0f;
    return ROVER_OK;
}

size_t rover_rollout_hparams_bytes(void) { return sizeof(rover_rollout_hparams); }

int rover_rollout_act(const rover_policy_desc *actor, const float *packed_a, const rover_policy_desc *critic, const float *packed_b,
                      int32_t n_copies, const rover_rollout_hparams *h, uint64_t counter, const float *obs, int32_t n,
                      const float *log_std, float *obs_out, float *mean_out, float *val_out, float *act_out, float *env_act_out,
                      float *logp_out, float *eps_out, void *stream)
{
    if (!actor || !critic || !h) return rover_internal_fail(ROVER_ERR_INVALID, "rover_rollout_act: NULL descriptor / hparams");
    if (!packed_a || !packed_b || !obs || !log_std || !mean_out || !val_out)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_rollout_act: NULL required pointer");
    if (n < 1 || n_copies < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_rollout_act: n and n_copies must be >= 1");
    if ((reinterpret_cast<uintptr_t>(packed_a) | reinterpret_cast<uintptr_t>(packed_b)) & 15)
        return rover_internal_fail(ROVER_ERR_INVALID, "packed weights must be 16-byte aligned");
    if (!(h->log_std_min <= h->log_std_max)) return rover_internal_fail(ROVER_ERR_INVALID, "rover_rollout_act: log_std_min > log_std_max");
    if (h->clip_actions && !(h->action_low <= h->action_high))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_rollout_act: action_low > action_high");
    if (obs_out == obs) return rover_internal_fail(ROVER_ERR_INVALID, "rover_rollout_act: obs_out must not alias obs");
    if (!is_reference_architecture(actor) || !is_reference_architecture(critic))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "rover_rollout_act: both networks must have the reference architecture");
    if (actor->leaky_slope != critic->leaky_slope)
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "rover_rollout_act: the two networks use different leaky-ReLU slopes");
    RolLaunch L;
    L.n_copies = n_copies;
    L.copy_floats_a = (unsigned)rover_policy_packed_floats(actor);
    L.copy_floats_b = (unsigned)rover_policy_packed_floats(critic);
    L.hp = *h;
    L.ctr_lo = (uint32_t)(counter & 0xFFFFFFFFu);
    L.ctr_hi = (uint32_t)(counter >> 32);
    L.log_std = log_std;
    L.obs_out = obs_out; L.mean_out = mean_out; L.val_out = val_out;
    L.act_out = act_out; L.env_act_out = env_act_out; L.logp_out = logp_out; L.eps_out = eps_out;
    // ROVER_ROLLOUT_PLAIN_STORE=1: the sanitised rows leave with a plain store (A/B measurement of the non-temporal one)
    static const bool plain = getenv("ROVER_ROLLOUT_PLAIN_STORE") != nullptr && getenv("ROVER_ROLLOUT_PLAIN_STORE")[0] == '1';
    const void *kfn = plain ? reinterpret_cast<const void *>(rover_rollout_act_kernel<false>)
                            : reinterpret_cast<const void *>(rover_rollout_act_kernel<true>);
    hipError_t e = hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    const dim3 grid(ceil_div(n, ROL_ROWS)), block(ROL_THREADS);
    if (plain)
        hipLaunchKernelGGL(rover_rollout_act_kernel<false>, grid, block, LDS_BYTES, static_cast<hipStream_t>(stream), *actor, *critic, L,
                           packed_a, packed_b, obs, n);
    else
        hipLaunchKernelGGL(rover_rollout_act_kernel<true>, grid, block, LDS_BYTES, static_cast<hipStream_t>(stream), *actor, *critic, L,
                           packed_a, packed_b, obs, n);
    e = hipGetLastError();
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "rover_rollout_act_kernel launch: %s", hipGetErrorString(e));
    return ROVER_OK;
}

int rover_rollout_record(const float *rew, const uint8_t *terminated, const uint8_t *truncated, int32_t n, float *rew_out,
                         float *done_out, void *stream)
{
    if (!rew || !terminated || !truncated || !rew_out || !done_out)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_rollout_record: NULL pointer");
    if (n < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_rollout_record: n must be >= 1");
    hipLaunchKernelGGL(rover_rollout_record_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), rew,
                       terminated, truncated, n, rew_out, done_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "rover_rollout_record_kernel launch: %s", hipGetErrorString(e));
    return ROVER_OK;
}

int rover_rollout_record_shaped(const float *rew, const uint8_t *terminated, const uint8_t *truncated, const float *val, int32_t n,
                                float reward_scale, float discount, int32_t time_limit_bootstrap, float *rew_out, float *done_out,
                                void *stream)
{
    if (!rew || !terminated || !truncated || !rew_out || !done_out)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_rollout_record_shaped: NULL pointer");
    if (time_limit_bootstrap && !val)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_rollout_record_shaped: val is NULL with time_limit_bootstrap");
    if (n < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_rollout_record_shaped: n must be >= 1");
    if ((reinterpret_cast<uintptr_t>(rew) | reinterpret_cast<uintptr_t>(val) | reinterpret_cast<uintptr_t>(rew_out) |
         reinterpret_cast<uintptr_t>(done_out)) & 3)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_rollout_record_shaped: float arrays must be 4-byte aligned");
    hipLaunchKernelGGL(rover_rollout_record_shaped_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), rew,
                       terminated, truncated, val, n, reward_scale, discount, time_limit_bootstrap != 0, rew_out, done_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "rover_rollout_record_shaped_kernel launch: %s", hipGetErrorString(e));
    return ROVER_OK;
}

}  // extern "C"
