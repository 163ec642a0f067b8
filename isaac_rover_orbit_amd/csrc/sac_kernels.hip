// sac_kernels.hip -- fused SAC update of the rover's Gaussian actor, twin critics and entropy coefficient (gfx950 / CDNA4,
// wave64).
//
// skrl SAC._update for the reference's tanh actor with a state-independent log_std and the Q(s, a) critic; see
// include/rover_sac.h for the contract and the reduction order.  The networks run layer by layer over the sampled rows, every
// dense product on v_mfma_f32_16x16x4_f32, in the pattern of td3_kernels.hip (restated here; that file is not shared):
//   sac_dense_kernel    Z = A W^T + b, act(Z) for up to 4 networks per launch (blockIdx.z): one wave per 16 rows x 64
//                       columns; the packed weights are the B fragments as they lie.  Layer 2 also writes the MLP input's
//                       proprioceptive columns and, for a critic, its two action columns;
//   sac_back_kernel     reverse dA = dZ W (times LeakyReLU' of the stored activation, or not: the action columns), up to 2
//                       networks per launch;
//   sac_wgrad_kernel    dW = dZ^T A and db = sum dZ per (16 x 16 tile, 512-row chunk) over up to 12 layers (both critics);
//   sac_combine_kernel  the chunk partials added in chunk order;
// plus the gather of the sampled rows from the observation ring, the one-thread-per-row heads (the Gaussian sample and its
// log-probability, y, the min of the critics, the Gaussian head's closed-form backward), fixed-order reductions into the
// device state, Adam and Polyak.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_hip.h"
#include "../../include/rover_policy.h"
#include "../../include/rover_sac.h"
#include "rover_internal.hpp"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int OBS = 965, PROP = 4, ENC_OFF = 3;
constexpr int ACOL = 64;                                     // first action column of the critic's MLP input
constexpr int NL = 6;
constexpr int AK[NL] = {961, 80, 64, 256, 160, 128};         // in features of the actor's layers
constexpr int CK[NL] = {961, 80, 66, 256, 160, 128};         // ... of the critic's (MLP input [prop, enc, a])
constexpr int LN[NL - 1] = {80, 60, 256, 160, 128};          // out features of layers 1 .. 5 (layer 6: 2 actor, 1 critic)
constexpr int FT = 256;                                      // threads of every multi-thread kernel here
constexpr int CH = 512;                                      // rows per weight-gradient chunk
constexpr int MAXZ = 4;                                      // networks per dense launch
constexpr int MAXJ = 2 * NL;                                 // layers per weight-gradient launch
// per-row matrices of one network (output of layer l, pitch MW[l]; layer 2's output sits at columns 4 .. 63 of the MLP
// input M, whose columns 64, 65 hold a critic's action)
constexpr int MW[NL] = {80, 68, 256, 160, 128, 4};
constexpr int ROW_F = 80 + 68 + 256 + 160 + 128 + 4;        // 696
constexpr int NSUM = 5;                                      // per-row sums of the critic head
constexpr int NPSUM = 4;                                     // ... of the policy head: loss, logp, dL/dls (2)
constexpr int RP = 8;                                        // stride of a block's partials
constexpr int HD = 8;                                        // Gaussian head's per-row record: u (2), mu (2), t (2), p (2)
constexpr int GP = 4;                                        // dL/du per row: critic_1's (2), critic_2's (2)
constexpr int TAIL = 8;                                      // log_std (2 + 2 pad), log_alpha (1 + 3 pad)
constexpr float LS_MIN = -20.0f, LS_MAX = 2.0f, U_MIN = -1.0f, U_MAX = 1.0f;
constexpr float HALF_LN_2PI = 0.91893853320467274178f;

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ inline size_t al4(size_t n) { return (n + 3) & ~(size_t)3; }

// fixed halving tree over the 256 threads of the block; the total in every thread after the call
__device__ __forceinline__ float block_sum(float v, float *red)
{
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = FT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// Cephes expf / tanhf as explicit fp32 sequences: the same text as policy_kernels.hip and ppo_kernels.hip
__device__ __forceinline__ float rv_expf(float x)
{
    if (x > 88.0f) return INFINITY;
    if (x < -88.0f) return 0.0f;
    const float z = floorf(1.44269504088896341f * x + 0.5f);
    x = x - z * 0.693359375f;
    x = x - z * -2.12194440e-4f;
    const float zz = x * x;
    float p = 1.9875691500e-4f;
    p = p * x + 1.3981999507e-3f;
    p = p * x + 8.3334519073e-3f;
    p = p * x + 4.1665795894e-2f;
    p = p * x + 1.6666665459e-1f;
    p = p * x + 5.0000001201e-1f;
    p = p * zz + x + 1.0f;
    return ldexpf(p, (int)z);
}
__device__ __forceinline__ float rv_tanhf(float x)
{
    const float z = fabsf(x);
    if (z > 44.0f) return x > 0.0f ? 1.0f : -1.0f;
    if (z >= 0.625f) {
        const float s = rv_expf(z + z);
        const float r = 1.0f - 2.0f / (s + 1.0f);
        return x < 0.0f ? -r : r;
    }
    if (x == 0.0f) return x;
    const float s = x * x;
    float p = -5.70498872745e-3f;
    p = p * s + 2.06390887954e-2f;
    p = p * s - 5.37397155531e-2f;
    p = p * s + 1.33314422036e-1f;
    p = p * s - 3.33332819422e-1f;
    return p * s * x + x;
}

// torch.clamp: a NaN stays a NaN
__device__ __forceinline__ float tclamp(float x, float lo, float hi) { return x != x ? x : fminf(fmaxf(x, lo), hi); }
// torch.min: NaN if either is NaN
__device__ __forceinline__ float tmin(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (a < b ? a : b); }
// the entropy coefficient from the parameter vector's log_alpha
__device__ __forceinline__ float alpha_of(const float *log_alpha) { return (float)exp((double)log_alpha[0]); }

// ---- gather: the ring rows of s and s' (64-bit row numbers) and the stored transition of every sampled row
struct GatherArgs {
    const int64_t *idx; int n; int64_t valid;
    int num_envs, slots;
    const int32_t *pos;
    const float *act, *rew; const uint8_t *term;     // NULL for the policy step
    int64_t *ro_s, *ro_n;
    float *a, *r, *nt;
    rover_sac_state *st;
};
__global__ __launch_bounds__(FT) void sac_gather_kernel(GatherArgs A)
{
    const int row = blockIdx.x * FT + threadIdx.x;
    if (row >= A.n) return;
    int64_t i = A.idx[row];
    bool bad = i < 0 || i >= A.valid;
    if (bad) i = 0;
    const int64_t k = i / A.num_envs, e = i - k * A.num_envs;
    int32_t p = A.pos[k];
    if (p < 0 || p >= A.slots) { bad = true; p = 0; }
    if (bad) A.st->bad_index = 1;                       // every writer stores the same word
    A.ro_s[row] = (int64_t)p * A.num_envs + e;
    A.ro_n[row] = (int64_t)(p + 1 == A.slots ? 0 : p + 1) * A.num_envs + e;
    if (A.act) {
        A.a[2 * (size_t)row] = A.act[2 * i];
        A.a[2 * (size_t)row + 1] = A.act[2 * i + 1];
        A.r[row] = A.rew[i];
        A.nt[row] = A.term[i] ? 0.0f : 1.0f;
    }
}

// ---- dense layer forward, one network per blockIdx.z
enum { ACT_NONE_ = 0, ACT_LEAKY_ = 1 };
struct Dense {
    const float *x; int xp;        // input A: row r at x + (ro ? ro[r] : r) * xp
    const int64_t *ro;
    const float *W, *b;            // packed weights / bias
    float *out; int op, ocol;      // output matrix, pitch, first column
    const float *prop;             // layer 2: M[r][0 .. 4) = prop[pro[r] * OBS + c] (the observation ring)
    const int64_t *pro;
    const float *ain; int aip;     // layer 2 of a critic: M[r][64 + c] = ain[r * aip + c]
    int K, N, act;
};
struct DenseLaunch {
    Dense d[MAXZ];
    int rows;
    float slope;
};
__global__ __launch_bounds__(FT) void sac_dense_kernel(DenseLaunch L)
{
    const Dense &A = L.d[blockIdx.z];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rr = lane >> 4, cc = lane & 15;
    const int r0 = blockIdx.x * 64 + wave * 16, t0 = blockIdx.y * 4;    // first row, first 16-column tile
    const int G = cdiv(A.K, 16), NT = cdiv(A.N, 16);
    if (A.prop && blockIdx.y == 0) {                                     // the proprioceptive (and action) columns of M
        const int r = r0 + (lane >> 2), c = lane & 3;
        if (r < L.rows) {
            A.out[(size_t)r * A.op + c] = A.prop[(size_t)A.pro[r] * OBS + c];
            if (A.ain && c < 2) A.out[(size_t)r * A.op + ACOL + c] = A.ain[(size_t)r * A.aip + c];
        }
    }
    const int ra = r0 + cc;                                              // the A operand's row of this lane
    const bool row_ok = ra < L.rows;
    const float *xrow = row_ok ? A.x + (A.ro ? (size_t)A.ro[ra] : (size_t)ra) * A.xp : nullptr;
    v4f acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    // sum_k a[r][k] * W[n][k] with W's packed fragments: lane (n & 15) + 16 (k & 3) of fragment (n / 16, k / 16) holds
    // W[n][16 g + 4 e + (k & 3)] in element e, exactly the B operand (k = rr, j = cc) of the 4 MFMAs of a 16-k group
    for (int g = 0; g < G; ++g) {
        float a[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = 16 * g + 4 * e + rr;
            a[e] = (xrow && k < A.K) ? xrow[k] : 0.0f;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t0 + t < NT) {
                const v4f w = reinterpret_cast<const v4f *>(A.W)[((size_t)(t0 + t) * G + g) * 64 + cc + 16 * rr];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], w[e], acc[t], 0, 0, 0);
            }
        }
    }
    // D[i][j]: lane holds i = 4 rr + jj, j = cc
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = 16 * (t0 + t) + cc;
        if (t0 + t >= NT || col >= A.N) continue;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int r = r0 + 4 * rr + jj;
            if (r >= L.rows) continue;
            const float s = acc[t][jj] + A.b[col];
            A.out[(size_t)r * A.op + A.ocol + col] = A.act == ACT_LEAKY_ ? (s > 0.0f ? s : s * L.slope) : s;
        }
    }
}

// ---- reverse: out[r][k - ocol] = (sum_n dZ[r][n] W[n][k]) * LeakyReLU'(aref[r][k]) (aref NULL: no derivative) for k in
// [k0, k0 + nk), one network per blockIdx.z
struct Back {
    const float *dz; int dzp;      // dZ of layer l (rows, N)
    const float *W; int K, N;      // packed weights of layer l (N x K)
    const float *aref; int arp;    // stored input activation of layer l, or NULL
    float *out; int op, ocol;
    int k0, nk;
};
struct BackLaunch {
    Back d[2];
    int rows;
    float slope;
};
__device__ __forceinline__ float w_at(const float *Wp, int G, int n, int k)
{
    return Wp[((((size_t)(n >> 4) * G + (k >> 4)) * 64 + (n & 15) + 16 * (k & 3)) << 2) + ((k >> 2) & 3)];
}
__global__ __launch_bounds__(FT) void sac_back_kernel(BackLaunch L)
{
    const Back &A = L.d[blockIdx.z];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rr = lane >> 4, cc = lane & 15;
    const int r0 = blockIdx.x * 64 + wave * 16, c0 = blockIdx.y * 64;    // first row, first output column (relative to k0)
    const int G = cdiv(A.K, 16);
    const int ra = r0 + cc;
    const bool row_ok = ra < L.rows;
    v4f acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    for (int nb = 0; nb < A.N; nb += 4) {
        const int n = nb + rr;
        const float a = (row_ok && n < A.N) ? A.dz[(size_t)ra * A.dzp + n] : 0.0f;   // A operand (i = cc, k = rr)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int kc = c0 + 16 * t + cc;                                           // B operand (k = rr, j = cc)
            const float w = (n < A.N && kc < A.nk) ? w_at(A.W, G, n, A.k0 + kc) : 0.0f;
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w, acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int kc = c0 + 16 * t + cc;
        if (kc >= A.nk) continue;
        const int k = A.k0 + kc;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int r = r0 + 4 * rr + jj;
            if (r >= L.rows) continue;
            const float d = acc[t][jj];
            A.out[(size_t)r * A.op + (k - A.ocol)] = (!A.aref || A.aref[(size_t)r * A.arp + k] > 0.0f) ? d : d * L.slope;
        }
    }
}

// ---- weight / bias gradients: one wave per (layer, 16 x 16 tile of the packed weights or a 16-row bias tile, chunk)
struct WgradArgs {
    const float *am[MAXJ]; int ap[MAXJ];      // input of layer j: row r at am + (ro ? ro[r] : r) * ap
    const int64_t *ro[MAXJ];
    const float *dz[MAXJ]; int dzp[MAXJ];     // dZ of layer j, pitch
    int K[MAXJ], N[MAXJ];
    uint32_t w_off[MAXJ], b_off[MAXJ];        // packed offsets relative to the block the partials cover
    int jobs[MAXJ + 1];                       // prefix sums of the per-layer job counts
    int nl, rows, P;                          // layers; rows; floats of the block (the partial's stride)
    float *part;                              // (chunks, P)
};
__global__ __launch_bounds__(FT) void sac_wgrad_kernel(WgradArgs A)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int job = blockIdx.x * 4 + wave;
    if (job >= A.jobs[A.nl]) return;
    int l = 0;
    while (job >= A.jobs[l + 1]) ++l;
    job -= A.jobs[l];
    const int K = A.K[l], N = A.N[l], G = cdiv(K, 16);
    const int t = job / (G + 1), g = job - t * (G + 1);
    const bool bias = g == G;
    const int rr = lane >> 4, cc = lane & 15;
    const int col = 16 * t + cc, kin = 16 * g + cc;
    const bool col_ok = col < N, k_ok = !bias && kin < K;
    const int rb0 = blockIdx.y * CH, rb1 = min(rb0 + CH, A.rows);
    const float *dz = A.dz[l], *am = A.am[l];
    const int64_t *ro = A.ro[l];
    const int dzp = A.dzp[l], ap = A.ap[l];
    v4f acc = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    // A operand: lane (i = cc, k = rr) = dZ[row][16 t + cc]; B operand: lane (k = rr, j = cc) = A[row][16 g + cc]
    for (int rb = rb0; rb < rb1; rb += 4) {
        const int r = rb + rr;
        const bool ok = r < rb1;
        const float a = ok && col_ok ? dz[(size_t)r * dzp + col] : 0.0f;
        float b;
        if (bias) b = ok ? 1.0f : 0.0f;
        else b = ok && k_ok ? am[(ro ? (size_t)ro[r] : (size_t)r) * ap + kin] : 0.0f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
    float *part = A.part + (size_t)blockIdx.y * A.P;
    // lane holds D[i = 4 rr + jj][j = cc] = dW[16 t + i][16 g + j]
    if (!bias) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int i = 4 * rr + jj, j = cc;
            const bool ok = 16 * t + i < N && 16 * g + j < K;
            // packed position: lane' = i + 16 (j & 3), element j >> 2
            part[A.w_off[l] + (((size_t)t * G + g) * 64 + i + 16 * (j & 3)) * 4 + (j >> 2)] = ok ? acc[jj] : 0.0f;
        }
    } else if (cc == 0) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int c = 16 * t + 4 * rr + jj;
            if (c < ((N + 3) & ~3)) part[A.b_off[l] + c] = c < N ? acc[jj] : 0.0f;
        }
    }
}

// out[e] = sum_c part[c][e] (c ascending) for e < P
__global__ __launch_bounds__(FT) void sac_combine_kernel(const float *part, int nch, int P, float *out)
{
    const int e = blockIdx.x * FT + threadIdx.x;
    if (e >= P) return;
    float s = part[e];
    for (int c = 1; c < nch; ++c) s += part[(size_t)c * P + e];
    out[e] = s;
}

// ---- Gaussian head (skrl GaussianMixin.act on a given draw): per row and component mu = tanh(z6), x = mu + sigma eps,
// u = clamp(x), t = (u - mu) / sigma, p = 1[-1 <= x <= 1] into hd, logp = sum_c(-0.5 t^2 - ls - ln(2 pi) / 2) into logp
struct GaussHead {
    const float *z6;               // the actor's last-layer output before tanh, pitch 4
    const float *log_std;          // 2 floats of the parameter vector
    const float *eps; int ecol;    // (rows, 4) draws, first column of this step's pair
    float *hd, *logp;
    int rows;
};
__global__ __launch_bounds__(FT) void sac_gauss_head_kernel(GaussHead A)
{
    const int r = blockIdx.x * FT + threadIdx.x;
    if (r >= A.rows) return;
    float lp = 0.0f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float mu = rv_tanhf(A.z6[(size_t)r * MW[NL - 1] + c]);
        const float ls = tclamp(A.log_std[c], LS_MIN, LS_MAX);
        const float sigma = rv_expf(ls);
        const float x = mu + sigma * A.eps[(size_t)r * 4 + A.ecol + c];
        const float u = tclamp(x, U_MIN, U_MAX);
        const float t = (u - mu) / sigma;
        float *h = A.hd + (size_t)r * HD;
        h[c] = u; h[2 + c] = mu; h[4 + c] = t; h[6 + c] = (x >= U_MIN && x <= U_MAX) ? 1.0f : 0.0f;
        lp += (-0.5f * (t * t) - ls) - HALF_LN_2PI;
    }
    A.logp[r] = lp;
}

// ---- critic head: y, the per-row squared errors and the critics' dZ6; block partials (fixed tree) to rowp[block * RP + i]
struct CriticHead {
    const float *tq1, *tq2, *q1, *q2;   // last-layer outputs, pitch 4
    const float *r, *nt, *logp;
    const float *log_alpha;
    float gamma, inv_n;
    float *dz1, *dz2;                   // dZ6 of critic_1 / critic_2, pitch 4
    float *y_out;
    int rows;
    float *rowp;
};
__global__ __launch_bounds__(FT) void sac_critic_head_kernel(CriticHead A)
{
    __shared__ float red[FT];
    const int r = blockIdx.x * FT + threadIdx.x;
    const float alpha = alpha_of(A.log_alpha);
    float t[NSUM] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (r < A.rows) {
        const size_t o = (size_t)r * MW[NL - 1];
        const float mq = tmin(A.tq1[o], A.tq2[o]) - alpha * A.logp[r];
        const float y = A.r[r] + (A.gamma * A.nt[r]) * mq;     // rewards + gamma * !terminated * (min(tq1, tq2) - alpha logp')
        const float e1 = A.q1[o] - y, e2 = A.q2[o] - y;
        A.dz1[o] = e1 * A.inv_n;                                // d/dq of (mse1 + mse2) / 2
        A.dz2[o] = e2 * A.inv_n;
        if (A.y_out) A.y_out[r] = y;
        t[0] = e1 * e1; t[1] = e2 * e2; t[2] = A.q1[o]; t[3] = A.q2[o]; t[4] = y;
    }
    for (int i = 0; i < NSUM; ++i) {
        const float tot = block_sum(t[i], red);
        if (threadIdx.x == 0) A.rowp[(size_t)blockIdx.x * RP + i] = tot;
    }
}

// ---- min head of the policy step: dZ6 of critic k = -w_k / B, w = (1, 0) where q1 < q2, (0, 1) where q2 < q1, (0.5, 0.5) on
// a tie (torch.min's backward); min(q1, q2) per row to minq
__global__ __launch_bounds__(FT) void sac_min_head_kernel(const float *q1, const float *q2, float *dz1, float *dz2, float *minq,
                                                          float inv_n, int rows)
{
    const int r = blockIdx.x * FT + threadIdx.x;
    if (r >= rows) return;
    const size_t o = (size_t)r * MW[NL - 1];
    const float a = q1[o], b = q2[o];
    const float w1 = a < b ? 1.0f : (a == b ? 0.5f : 0.0f);
    const float w2 = b < a ? 1.0f : (a == b ? 0.5f : 0.0f);
    dz1[o] = -(w1 * inv_n);
    dz2[o] = -(w2 * inv_n);
    minq[r] = tmin(a, b);
}

// ---- Gaussian backward head (the closed form of sac.gaussian_head_backward): with g = d(-min q / B)/du = g1 + g2 from the
// critics' reverse,
//   dL/dmu = alpha t / sigma (1 - p) / B + p g,  dL/dls = alpha (t^2 - 1 - p t eps) / B + p g sigma eps,  dL/dz6 = dL/dmu (1 - mu^2)
// and the block partials of (alpha logp - min q, logp, dL/dls[0], dL/dls[1])
struct GaussBack {
    const float *hd, *logp, *minq, *g;
    const float *log_std, *log_alpha;
    const float *eps; int ecol;
    float inv_n;
    float *dz6;                         // the actor's dZ6, pitch 4
    float *u_out, *logp_out, *dmean_out;
    int rows;
    float *rowp;
};
__global__ __launch_bounds__(FT) void sac_gauss_back_kernel(GaussBack A)
{
    __shared__ float red[FT];
    const int r = blockIdx.x * FT + threadIdx.x;
    const float alpha = alpha_of(A.log_alpha);
    float t4[NPSUM] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (r < A.rows) {
        const float *h = A.hd + (size_t)r * HD;
        const float lp = A.logp[r];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float sigma = rv_expf(tclamp(A.log_std[c], LS_MIN, LS_MAX));
            const float u = h[c], mu = h[2 + c], t = h[4 + c], p = h[6 + c];
            const float e = A.eps[(size_t)r * 4 + A.ecol + c];
            const float g = (A.g[(size_t)r * GP + c] + A.g[(size_t)r * GP + 2 + c]) * p;
            const float dmu = (alpha * (t / sigma) * (1.0f - p)) * A.inv_n + g;
            const float dls = (alpha * (t * t - 1.0f - p * t * e)) * A.inv_n + g * (sigma * e);
            A.dz6[(size_t)r * MW[NL - 1] + c] = dmu * (1.0f - mu * mu);
            if (A.u_out) A.u_out[2 * (size_t)r + c] = u;
            if (A.dmean_out) A.dmean_out[2 * (size_t)r + c] = dmu;
            t4[2 + c] = dls;
        }
        if (A.logp_out) A.logp_out[r] = lp;
        t4[0] = alpha * lp - A.minq[r];
        t4[1] = lp;
    }
    for (int i = 0; i < NPSUM; ++i) {
        const float tot = block_sum(t4[i], red);
        if (threadIdx.x == 0) A.rowp[(size_t)blockIdx.x * RP + i] = tot;
    }
}

// thread t adds partials t, t + 256, ... in order, then the tree; total of row-term i in tot[i] (every thread)
__device__ void reduce_rows(const float *rowp, int nblk, int nterms, float *tot, float *red)
{
    for (int i = 0; i < nterms; ++i) {
        float s = 0.0f;
        for (int b = threadIdx.x; b < nblk; b += FT) s += rowp[(size_t)b * RP + i];
        tot[i] = block_sum(s, red);
    }
}
__device__ void adam_scalars(int step, float beta1, float beta2, float lr, float *step_size, float *bc2_sqrt)
{
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    *step_size = (float)((double)lr / bc1);
    *bc2_sqrt = (float)sqrt(bc2);
}
__global__ __launch_bounds__(FT) void sac_critic_final_kernel(const float *rowp, int nblk, float inv_n, float beta1, float beta2, float lr,
                                                              rover_sac_state *st)
{
    __shared__ float red[FT];
    float tot[NSUM];
    reduce_rows(rowp, nblk, NSUM, tot, red);
    if (threadIdx.x == 0) {
        st->critic_loss = (tot[0] * inv_n + tot[1] * inv_n) * 0.5f;
        st->q1_mean = tot[2] * inv_n;
        st->q2_mean = tot[3] * inv_n;
        st->y_mean = tot[4] * inv_n;
        st->critic_step += 1;
        adam_scalars(st->critic_step, beta1, beta2, lr, &st->critic_step_size, &st->critic_bc2_sqrt);
    }
}
// the policy step's one final workgroup: the losses and means, the gradients of log_std (under the clamp mask) and log_alpha,
// exact zeros into the padding of the gradient's tail, the step counters and Adam scalars of the policy and the entropy step
struct PolicyFinal {
    const float *rowp; int nblk;
    float inv_n, beta1, beta2, actor_lr, entropy_lr, target_entropy;
    int learn_entropy;
    const float *tail_p;                // log_std, log_alpha of the parameter vector
    float *tail_g; int tail_n;          // the gradient's tail: TAIL floats and the padding behind them
    rover_sac_state *st;
};
__global__ __launch_bounds__(FT) void sac_policy_final_kernel(PolicyFinal A)
{
    __shared__ float red[FT];
    float tot[NPSUM];
    reduce_rows(A.rowp, A.nblk, NPSUM, tot, red);
    for (int e = TAIL + threadIdx.x; e < A.tail_n; e += FT) A.tail_g[e] = 0.0f;
    if (threadIdx.x == 0) {
        rover_sac_state *st = A.st;
        const float log_alpha = A.tail_p[4];
        const float logp_mean = tot[1] * A.inv_n;
        st->policy_loss = tot[0] * A.inv_n;
        st->logp_mean = logp_mean;
        st->alpha = alpha_of(A.tail_p + 4);
        for (int c = 0; c < 2; ++c) {
            const float ls = A.tail_p[c];
            A.tail_g[c] = (ls >= LS_MIN && ls <= LS_MAX) ? tot[2 + c] : 0.0f;     // clamp's backward
            A.tail_g[2 + c] = 0.0f;
        }
        for (int c = 4; c < TAIL; ++c) A.tail_g[c] = 0.0f;
        st->actor_step += 1;
        adam_scalars(st->actor_step, A.beta1, A.beta2, A.actor_lr, &st->actor_step_size, &st->actor_bc2_sqrt);
        if (A.learn_entropy) {
            const float d = logp_mean + A.target_entropy;
            st->entropy_loss = -(log_alpha * d);
            A.tail_g[4] = -d;
            st->entropy_step += 1;
            adam_scalars(st->entropy_step, A.beta1, A.beta2, A.entropy_lr, &st->entropy_step_size, &st->entropy_bc2_sqrt);
        }
    }
}

// ---- Adam (torch's single-tensor order) over P floats; sc = {step_size, bc2_sqrt} in the state; then the replicas
__device__ __forceinline__ float adam_one(float *params, const float *grad, float *m, float *v, const float *sc, int e, float beta1,
                                          float beta2, float eps)
{
    const float g = grad[e];
    const float w1 = (float)(1.0 - (double)beta1), w2 = (float)(1.0 - (double)beta2);
    const float mo = m[e], mn = mo + w1 * (g - mo);                     // exp_avg.lerp_(grad, 1 - beta1)
    const float vn = v[e] * beta2 + w2 * (g * g);                       // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    const float denom = sqrtf(vn) / sc[1] + eps;                        // (exp_avg_sq.sqrt() / sqrt(bc2)).add_(eps)
    const float p = params[e] + (-sc[0]) * (mn / denom);                // param.addcdiv_(exp_avg, denom, -lr / bc1)
    m[e] = mn;
    v[e] = vn;
    params[e] = p;
    return p;
}
__global__ __launch_bounds__(FT) void sac_adam_kernel(float *params, const float *grad, float *m, float *v, const float *sc, int P,
                                                      float beta1, float beta2, float eps, float *rep, int n_copies)
{
    const int e = blockIdx.x * FT + threadIdx.x;
    if (e >= P) return;
    const float p = adam_one(params, grad, m, v, sc, e, beta1, beta2, eps);
    if (rep)
        for (int c = 0; c < n_copies; ++c) rep[(size_t)c * P + e] = p;
}
// the tail: log_std (floats 0 .. 3) with the policy's scalars, log_alpha (floats 4 .. 7) with the entropy step's, if it is learned
__global__ __launch_bounds__(64) void sac_tail_adam_kernel(float *params, const float *grad, float *m, float *v, const float *sc_actor,
                                                           const float *sc_entropy, int learn_entropy, float beta1, float beta2, float eps)
{
    const int e = threadIdx.x;
    if (e >= TAIL) return;
    if (e >= 4 && !learn_entropy) return;
    adam_one(params, grad, m, v, e < 4 ? sc_actor : sc_entropy, e, beta1, beta2, eps);
}

// ---- Polyak: t.mul_(1 - tau); t.add_(tau * p) -- two fp32 roundings per product, one per sum (no contraction)
__global__ __launch_bounds__(FT) void sac_polyak_kernel(float *t, const float *p, size_t count, float keep, float tau)
{
    const size_t e = (size_t)blockIdx.x * FT + threadIdx.x;
    if (e >= count) return;
    const float a = t[e] * keep;
    const float b = p[e] * tau;
    t[e] = a + b;
}

// ---- host side
size_t layer_weight_floats(int N, int K) { return (size_t)cdiv(N, 16) * cdiv(K, 16) * 64 * 4; }
size_t layer_bias_floats(int N) { return al4((size_t)N); }
int out_of(int l, bool critic) { return l < NL - 1 ? LN[l] : (critic ? 1 : 2); }
int in_of(int l, bool critic) { return critic ? CK[l] : AK[l]; }
size_t net_floats(bool critic)
{
    size_t n = 0;
    for (int l = 0; l < NL; ++l) n += layer_weight_floats(out_of(l, critic), in_of(l, critic)) + layer_bias_floats(out_of(l, critic));
    return n;
}
size_t tail_off() { return net_floats(false) + 2 * net_floats(true); }
size_t param_floats() { return (tail_off() + TAIL + 63) & ~(size_t)63; }

// the shapes and the offsets the pack sets of the tanh actor / the critic
bool is_net(const rover_policy_desc *d, bool critic)
{
    if (!d) return false;
    if (d->obs_dim != OBS || d->prop_dim != PROP || d->enc_offset != ENC_OFF || d->enc_dim != CK[0] || d->n_enc != 2 || d->n_mlp != 4)
        return false;
    if (d->leaky_slope != 0.01f) return false;
    size_t off = 0;
    for (int i = 0; i < NL; ++i) {
        const rover_policy_layer &l = d->layers[i];
        const int N = out_of(i, critic), K = in_of(i, critic);
        if (l.K != K || l.N != N) return false;
        if (l.act != (i < NL - 1 ? ROVER_ACT_LEAKY_RELU : (critic ? ROVER_ACT_NONE : ROVER_ACT_TANH))) return false;
        if ((l.split_k != 0) != (i == 0 || i == NL - 1)) return false;
        if (l.w_off != off) return false;
        off += layer_weight_floats(N, K);
        if (l.b_off != off) return false;
        off += layer_bias_floats(N);
    }
    return true;
}
int check_nets(const rover_policy_desc *actor, const rover_policy_desc *critic)
{
    if (!actor || !critic) return rover_internal_fail(ROVER_ERR_INVALID, "descriptor is NULL");
    if (!is_net(actor, false) || !is_net(critic, true))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "the fused SAC update runs the reference's tanh actor (rover_policy_default_desc(2, 1), "
                                                          "packed by rover_policy_pack) and the Q(s, a) critic (rover_td3_critic_desc, "
                                                          "packed by rover_td3_critic_pack) only");
    return ROVER_OK;
}

struct Net {
    const float *p;                  // the network's packed block
    uint32_t w_off[NL], b_off[NL];
    bool critic;
};
Net net_at(const rover_policy_desc *d, const float *block, bool critic)
{
    Net n;
    n.p = block;
    for (int i = 0; i < NL; ++i) { n.w_off[i] = d->layers[i].w_off; n.b_off[i] = d->layers[i].b_off; }
    n.critic = critic;
    return n;
}

// workspace layout: per-row vectors (ro_s, ro_n as int64; a (2), r, nt, y / min q, logp, the Gaussian head's record (HD), the
// critics' dL/du (GP) as float), row partials, then 5 network regions (cache + scratch, ROW_F floats per row each): 0 actor,
// 1 / 2 target critics, 3 / 4 critics; then the weight-gradient chunk partials of both critics
struct Region {
    float *cache[NL], *scr[NL];
};
constexpr int NREG = 5;
size_t rowp_floats(int rows) { return al4((size_t)RP * cdiv(rows, FT)); }
size_t part_floats(int rows) { return (size_t)cdiv(rows, CH) * (2 * net_floats(true)); }
size_t ws_bytes_for(int rows)
{
    const size_t R = (size_t)rows;
    size_t f = 4 * al4(R) /* ro_s, ro_n: 2 floats each */ + 2 * al4(R) + 4 * al4(R) + (HD + GP) * al4(R) + rowp_floats(rows) +
               NREG * 2 * (size_t)ROW_F * R + part_floats(rows);
    return sizeof(float) * f;
}
struct Ws {
    int64_t *ro_s, *ro_n;
    float *a, *r, *nt, *y, *logp, *hd, *g, *rowp, *part;
    Region reg[NREG];
};
Ws ws_at(void *ws, int rows)
{
    Ws w;
    const size_t R = (size_t)rows;
    float *f = static_cast<float *>(ws);
    w.ro_s = reinterpret_cast<int64_t *>(f); f += 2 * al4(R);
    w.ro_n = reinterpret_cast<int64_t *>(f); f += 2 * al4(R);
    w.a = f; f += 2 * al4(R);
    w.r = f; f += al4(R);
    w.nt = f; f += al4(R);
    w.y = f; f += al4(R);
    w.logp = f; f += al4(R);
    w.hd = f; f += HD * al4(R);
    w.g = f; f += GP * al4(R);
    w.rowp = f; f += rowp_floats(rows);
    for (int k = 0; k < NREG; ++k) {
        for (int s = 0; s < 2; ++s)
            for (int l = 0; l < NL; ++l) {
                (s ? w.reg[k].scr : w.reg[k].cache)[l] = f;
                f += (size_t)MW[l] * R;
            }
    }
    w.part = f;
    return w;
}

int device_of(const void *p, int *dev)
{
    hipPointerAttribute_t at;
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_INVALID, "not a device pointer: %s", hipGetErrorString(e));
    *dev = at.device;
    return ROVER_OK;
}
int launched(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, what, hipGetErrorString(e));
    return ROVER_OK;
}

// the forward of up to MAXZ networks over `rows` rows; net z reads observation rows ro[z] and (critics) actions ain[z] and
// writes its layer outputs to reg[z]->cache.  The actor's last layer is written before its tanh (the head applies it).
struct FwdJob {
    Net net;
    const int64_t *ro;
    const float *ain; int aip;
    Region *reg;
};
int forward(const FwdJob *jobs, int nz, const float *obs, int rows, hipStream_t s)
{
    for (int l = 0; l < NL; ++l) {
        DenseLaunch L = {};
        L.rows = rows;
        L.slope = 0.01f;
        int N = 0;
        for (int z = 0; z < nz; ++z) {
            const FwdJob &j = jobs[z];
            Dense &A = L.d[z];
            N = out_of(l, j.net.critic);
            if (l == 0) { A.x = obs + ENC_OFF; A.xp = OBS; A.ro = j.ro; }
            else { A.x = j.reg->cache[l - 1]; A.xp = MW[l - 1]; }
            A.W = j.net.p + j.net.w_off[l]; A.b = j.net.p + j.net.b_off[l];
            A.out = j.reg->cache[l]; A.op = MW[l]; A.ocol = l == 1 ? PROP : 0;
            if (l == 1) {
                A.prop = obs; A.pro = j.ro;
                if (j.net.critic) { A.ain = j.ain; A.aip = j.aip; }
            }
            A.K = in_of(l, j.net.critic); A.N = N;
            A.act = l < NL - 1 ? ACT_LEAKY_ : ACT_NONE_;
        }
        hipLaunchKernelGGL(sac_dense_kernel, dim3(cdiv(rows, 64), cdiv(N, 64), nz), dim3(FT), 0, s, L);
        if (int rc = launched("sac_dense_kernel launch: %s")) return rc;
    }
    return ROVER_OK;
}

// reverse of layer l for nz networks at once: dZ_{l-1} = (dZ_l W_l) * LeakyReLU'(a_{l-1}) into scr[l - 1]
int back_layer(const Net *nets, Region *const *regs, int nz, int l, int rows, hipStream_t s)
{
    BackLaunch L = {};
    L.rows = rows;
    L.slope = 0.01f;
    int nk = 0;
    for (int z = 0; z < nz; ++z) {
        Back &B = L.d[z];
        const Net &n = nets[z];
        B.dz = l == 1 ? regs[z]->scr[1] + PROP : regs[z]->scr[l]; B.dzp = MW[l];
        B.W = n.p + n.w_off[l]; B.K = in_of(l, n.critic); B.N = out_of(l, n.critic);
        B.aref = regs[z]->cache[l - 1]; B.arp = MW[l - 1];
        B.out = regs[z]->scr[l - 1]; B.op = MW[l - 1]; B.ocol = 0;
        B.k0 = l == 2 ? PROP : 0; B.nk = l == 2 ? LN[1] : in_of(l, n.critic);
        nk = B.nk;
    }
    hipLaunchKernelGGL(sac_back_kernel, dim3(cdiv(rows, 64), cdiv(nk, 64), nz), dim3(FT), 0, s, L);
    return launched("sac_back_kernel launch: %s");
}

// weight gradients of nz networks whose packed blocks lie back to back (block_floats each) into out[0 .. nz * block_floats)
int wgrad(const Net *nets, Region *const *regs, const int64_t *ro, int nz, const float *obs, int rows, float *part, float *out,
          hipStream_t s)
{
    WgradArgs W = {};
    const uint32_t bf = (uint32_t)net_floats(nets[0].critic);
    W.jobs[0] = 0;
    int j = 0;
    for (int z = 0; z < nz; ++z)
        for (int l = 0; l < NL; ++l, ++j) {
            const Net &n = nets[z];
            W.K[j] = in_of(l, n.critic); W.N[j] = out_of(l, n.critic);
            if (l == 0) { W.am[j] = obs + ENC_OFF; W.ap[j] = OBS; W.ro[j] = ro; }
            else { W.am[j] = regs[z]->cache[l - 1]; W.ap[j] = MW[l - 1]; W.ro[j] = nullptr; }
            // dZ of layer 2 (the encoder's 60 outputs) sits at columns 4 .. 63 of its 68-wide matrix
            W.dz[j] = l == 1 ? regs[z]->scr[1] + PROP : regs[z]->scr[l]; W.dzp[j] = MW[l];
            W.w_off[j] = z * bf + n.w_off[l]; W.b_off[j] = z * bf + n.b_off[l];
            W.jobs[j + 1] = W.jobs[j] + cdiv(W.N[j], 16) * (cdiv(W.K[j], 16) + 1);
        }
    W.nl = j; W.rows = rows; W.P = (int)(nz * bf); W.part = part;
    const int nch = cdiv(rows, CH);
    hipLaunchKernelGGL(sac_wgrad_kernel, dim3(cdiv(W.jobs[j], 4), nch), dim3(FT), 0, s, W);
    if (int rc = launched("sac_wgrad_kernel launch: %s")) return rc;
    hipLaunchKernelGGL(sac_combine_kernel, dim3(cdiv(W.P, FT)), dim3(FT), 0, s, (const float *)part, nch, W.P, out);
    return launched("sac_combine_kernel launch: %s");
}

int common_checks(const rover_policy_desc *actor, const rover_policy_desc *critic, const rover_sac_hparams *h, const void *params,
                  const void *grad, const void *adam_m, const void *adam_v, const float *obs_ring, int32_t slots, int32_t num_envs,
                  const int32_t *ring_pos, const int64_t *idx, int32_t n, int64_t valid_rows, const float *eps, const void *ws,
                  size_t ws_bytes, const void *state)
{
    if (int rc = check_nets(actor, critic)) return rc;
    if (!h || !params || !grad || !adam_m || !adam_v || !obs_ring || !ring_pos || !idx || !eps || !ws || !state)
        return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (n < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n must be >= 1");
    if (slots < 2 || num_envs < 1) return rover_internal_fail(ROVER_ERR_INVALID, "the ring needs >= 2 slots and >= 1 env");
    if (valid_rows < 1 || valid_rows > (int64_t)(slots - 1) * num_envs)
        return rover_internal_fail(ROVER_ERR_INVALID, "valid_rows must be in [1, (slots - 1) * num_envs]");
    if (ws_bytes < rover_sac_workspace_bytes(n)) return rover_internal_fail(ROVER_ERR_INVALID, "SAC workspace too small");
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grad) |
         reinterpret_cast<uintptr_t>(adam_m) | reinterpret_cast<uintptr_t>(adam_v)) & 15)
        return rover_internal_fail(ROVER_ERR_INVALID, "workspace and parameter vectors must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(state) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "state must be 8-byte aligned");
    return ROVER_OK;
}

int gather(const Ws &w, const int64_t *idx, int n, int64_t valid, int num_envs, int slots, const int32_t *pos, const float *act,
           const float *rew, const uint8_t *term, rover_sac_state *st, hipStream_t s)
{
    GatherArgs G = {};
    G.idx = idx; G.n = n; G.valid = valid; G.num_envs = num_envs; G.slots = slots; G.pos = pos;
    G.act = act; G.rew = rew; G.term = term;
    G.ro_s = w.ro_s; G.ro_n = w.ro_n; G.a = w.a; G.r = w.r; G.nt = w.nt; G.st = st;
    hipLaunchKernelGGL(sac_gather_kernel, dim3(cdiv(n, FT)), dim3(FT), 0, s, G);
    return launched("sac_gather_kernel launch: %s");
}

// the actor on the ring rows `ro` and its Gaussian head on eps[:, ecol .. ecol + 2): u, mu, t, p into w.hd, logp into w.logp
int act(const Ws &w, Region *reg, const Net &pi, const float *tail, const int64_t *ro, const float *obs, const float *eps, int ecol,
        int n, hipStream_t s)
{
    FwdJob ja = {pi, ro, nullptr, 0, reg};
    if (int rc = forward(&ja, 1, obs, n, s)) return rc;
    GaussHead H = {};
    H.z6 = reg->cache[NL - 1]; H.log_std = tail; H.eps = eps; H.ecol = ecol; H.hd = w.hd; H.logp = w.logp; H.rows = n;
    hipLaunchKernelGGL(sac_gauss_head_kernel, dim3(cdiv(n, FT)), dim3(FT), 0, s, H);
    return launched("sac_gauss_head_kernel launch: %s");
}

}  // namespace

extern "C" {

int rover_sac_default_hparams(rover_sac_hparams *h)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "hparams is NULL");
    h->gamma = 0.99f;
    h->polyak = 0.005f;
    h->actor_lr = 1e-4f; h->critic_lr = 1e-4f; h->entropy_lr = 5e-3f;
    h->beta1 = 0.9f; h->beta2 = 0.999f; h->eps = 1e-8f;
    h->target_entropy = -2.0f;
    h->learn_entropy = 1;
    return ROVER_OK;
}
size_t rover_sac_hparams_bytes(void) { return sizeof(rover_sac_hparams); }
size_t rover_sac_state_bytes(void) { return sizeof(rover_sac_state); }

size_t rover_sac_param_floats(const rover_policy_desc *actor, const rover_policy_desc *critic)
{
    if (!is_net(actor, false) || !is_net(critic, true)) return 0;
    return param_floats();
}
size_t rover_sac_workspace_bytes(int32_t max_rows) { return max_rows > 0 ? ws_bytes_for(max_rows) : 0; }

int rover_sac_critic_step(const rover_policy_desc *actor, const rover_policy_desc *critic, const rover_sac_hparams *h,
                          float *params, const float *target, float *grad, float *adam_m, float *adam_v, const float *obs_ring,
                          int32_t slots, int32_t num_envs, const int32_t *ring_pos, const float *act_mem, const float *rew,
                          const uint8_t *terminated, const int64_t *idx, int32_t n, int64_t valid_rows, const float *eps,
                          void *ws, size_t ws_bytes, void *state, float *y_out, void *stream)
{
    if (int rc = common_checks(actor, critic, h, params, grad, adam_m, adam_v, obs_ring, slots, num_envs, ring_pos, idx, n, valid_rows,
                               eps, ws, ws_bytes, state))
        return rc;
    if (!target || !act_mem || !rew || !terminated) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (reinterpret_cast<uintptr_t>(target) & 15) return rover_internal_fail(ROVER_ERR_INVALID, "target must be 16-byte aligned");
    int dev;
    if (int rc = device_of(params, &dev)) return rc;
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    rover_sac_state *st = static_cast<rover_sac_state *>(state);
    Ws w = ws_at(ws, n);
    const size_t Pa = net_floats(false), Pc = net_floats(true);
    const float *tail = params + tail_off();
    const Net pi = net_at(actor, params, false);
    const Net tq1 = net_at(critic, target, true), tq2 = net_at(critic, target + Pc, true);
    const Net q1 = net_at(critic, params + Pa, true), q2 = net_at(critic, params + Pa + Pc, true);
    if (int rc = gather(w, idx, n, valid_rows, num_envs, slots, ring_pos, act_mem, rew, terminated, st, s)) return rc;
    // (u', logp') = act(s', eps[:, 0:2])
    if (int rc = act(w, &w.reg[0], pi, tail, w.ro_n, obs_ring, eps, 0, n, s)) return rc;
    // target critics on (s', u') and critics on (s, a) in the same launches
    FwdJob jc[4] = {{tq1, w.ro_n, w.hd, HD, &w.reg[1]}, {tq2, w.ro_n, w.hd, HD, &w.reg[2]},
                    {q1, w.ro_s, w.a, 2, &w.reg[3]}, {q2, w.ro_s, w.a, 2, &w.reg[4]}};
    if (int rc = forward(jc, 4, obs_ring, n, s)) return rc;
    CriticHead H = {};
    H.tq1 = w.reg[1].cache[NL - 1]; H.tq2 = w.reg[2].cache[NL - 1]; H.q1 = w.reg[3].cache[NL - 1]; H.q2 = w.reg[4].cache[NL - 1];
    H.r = w.r; H.nt = w.nt; H.logp = w.logp; H.log_alpha = tail + 4; H.gamma = h->gamma; H.inv_n = 1.0f / (float)n;
    H.dz1 = w.reg[3].scr[NL - 1]; H.dz2 = w.reg[4].scr[NL - 1];
    H.y_out = y_out; H.rows = n; H.rowp = w.rowp;
    hipLaunchKernelGGL(sac_critic_head_kernel, dim3(cdiv(n, FT)), dim3(FT), 0, s, H);
    hipLaunchKernelGGL(sac_critic_final_kernel, dim3(1), dim3(FT), 0, s, (const float *)w.rowp, cdiv(n, FT), H.inv_n, h->beta1, h->beta2,
                       h->critic_lr, st);
    if (int rc = launched("sac critic head launch: %s")) return rc;
    // reverse of both critics, weight gradients into the critic blocks, Adam over both
    const Net qs[2] = {q1, q2};
    Region *regs[2] = {&w.reg[3], &w.reg[4]};
    for (int l = NL - 1; l >= 1; --l)
        if (int rc = back_layer(qs, regs, 2, l, n, s)) return rc;
    if (int rc = wgrad(qs, regs, w.ro_s, 2, obs_ring, n, w.part, grad + Pa, s)) return rc;
    hipLaunchKernelGGL(sac_adam_kernel, dim3(cdiv((int)(2 * Pc), FT)), dim3(FT), 0, s, params + Pa, (const float *)grad + Pa, adam_m + Pa,
                       adam_v + Pa, (const float *)&st->critic_step_size, (int)(2 * Pc), h->beta1, h->beta2, h->eps, (float *)nullptr, 0);
    return launched("sac_adam_kernel launch: %s");
}

int rover_sac_policy_step(const rover_policy_desc *actor, const rover_policy_desc *critic, const rover_sac_hparams *h,
                          float *params, float *grad, float *adam_m, float *adam_v, const float *obs_ring, int32_t slots,
                          int32_t num_envs, const int32_t *ring_pos, const int64_t *idx, int32_t n, int64_t valid_rows,
                          const float *eps, void *ws, size_t ws_bytes, void *state, float *replicas_actor, int32_t n_copies,
                          float *u_out, float *logp_out, float *dmean_out, void *stream)
{
    if (int rc = common_checks(actor, critic, h, params, grad, adam_m, adam_v, obs_ring, slots, num_envs, ring_pos, idx, n, valid_rows,
                               eps, ws, ws_bytes, state))
        return rc;
    if (replicas_actor && n_copies < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n_copies must be >= 1");
    int dev;
    if (int rc = device_of(params, &dev)) return rc;
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    rover_sac_state *st = static_cast<rover_sac_state *>(state);
    Ws w = ws_at(ws, n);
    const size_t Pa = net_floats(false), Pc = net_floats(true), To = tail_off();
    const float *tail = params + To;
    const Net pi = net_at(actor, params, false);
    const Net q1 = net_at(critic, params + Pa, true), q2 = net_at(critic, params + Pa + Pc, true);
    Region &RA = w.reg[0];
    const float inv_n = 1.0f / (float)n;
    if (int rc = gather(w, idx, n, valid_rows, num_envs, slots, ring_pos, nullptr, nullptr, nullptr, st, s)) return rc;
    // (u, logp) = act(s, eps[:, 2:4]), both critics on (s, u)
    if (int rc = act(w, &RA, pi, tail, w.ro_s, obs_ring, eps, 2, n, s)) return rc;
    FwdJob jq[2] = {{q1, w.ro_s, w.hd, HD, &w.reg[3]}, {q2, w.ro_s, w.hd, HD, &w.reg[4]}};
    if (int rc = forward(jq, 2, obs_ring, n, s)) return rc;
    hipLaunchKernelGGL(sac_min_head_kernel, dim3(cdiv(n, FT)), dim3(FT), 0, s, (const float *)w.reg[3].cache[NL - 1],
                       (const float *)w.reg[4].cache[NL - 1], w.reg[3].scr[NL - 1], w.reg[4].scr[NL - 1], w.y, inv_n, n);
    if (int rc = launched("sac_min_head_kernel launch: %s")) return rc;
    // both critics' MLP reverse down to their input M, then only the two action columns: critic k's dL/du into g[:, 2 k .. 2 k + 2)
    const Net qs[2] = {q1, q2};
    Region *regs[2] = {&w.reg[3], &w.reg[4]};
    for (int l = NL - 1; l >= 3; --l)
        if (int rc = back_layer(qs, regs, 2, l, n, s)) return rc;
    {
        BackLaunch L = {};
        L.rows = n; L.slope = 0.01f;
        for (int z = 0; z < 2; ++z) {
            Back &B = L.d[z];
            B.dz = regs[z]->scr[2]; B.dzp = MW[2];
            B.W = qs[z].p + qs[z].w_off[2]; B.K = CK[2]; B.N = LN[2];
            B.aref = nullptr; B.arp = 0;
            B.out = w.g; B.op = GP; B.ocol = ACOL - 2 * z;
            B.k0 = ACOL; B.nk = 2;
        }
        hipLaunchKernelGGL(sac_back_kernel, dim3(cdiv(n, 64), 1, 2), dim3(FT), 0, s, L);
        if (int rc = launched("sac_back_kernel launch: %s")) return rc;
    }
    GaussBack B = {};
    B.hd = w.hd; B.logp = w.logp; B.minq = w.y; B.g = w.g; B.log_std = tail; B.log_alpha = tail + 4; B.eps = eps; B.ecol = 2;
    B.inv_n = inv_n; B.dz6 = RA.scr[NL - 1]; B.u_out = u_out; B.logp_out = logp_out; B.dmean_out = dmean_out; B.rows = n;
    B.rowp = w.rowp;
    hipLaunchKernelGGL(sac_gauss_back_kernel, dim3(cdiv(n, FT)), dim3(FT), 0, s, B);
    if (int rc = launched("sac_gauss_back_kernel launch: %s")) return rc;
    // the actor's reverse and weight gradients into the actor block
    Region *ra[1] = {&RA};
    for (int l = NL - 1; l >= 1; --l)
        if (int rc = back_layer(&pi, ra, 1, l, n, s)) return rc;
    if (int rc = wgrad(&pi, ra, w.ro_s, 1, obs_ring, n, w.part, grad, s)) return rc;
    PolicyFinal F = {};
    F.rowp = w.rowp; F.nblk = cdiv(n, FT); F.inv_n = inv_n; F.beta1 = h->beta1; F.beta2 = h->beta2; F.actor_lr = h->actor_lr;
    F.entropy_lr = h->entropy_lr; F.target_entropy = h->target_entropy; F.learn_entropy = h->learn_entropy != 0;
    F.tail_p = tail; F.tail_g = grad + To; F.tail_n = (int)(param_floats() - To); F.st = st;
    hipLaunchKernelGGL(sac_policy_final_kernel, dim3(1), dim3(FT), 0, s, F);
    if (int rc = launched("sac_policy_final_kernel launch: %s")) return rc;
    hipLaunchKernelGGL(sac_adam_kernel, dim3(cdiv((int)Pa, FT)), dim3(FT), 0, s, params, (const float *)grad, adam_m, adam_v,
                       (const float *)&st->actor_step_size, (int)Pa, h->beta1, h->beta2, h->eps, replicas_actor, (int)n_copies);
    hipLaunchKernelGGL(sac_tail_adam_kernel, dim3(1), dim3(64), 0, s, params + To, (const float *)grad + To, adam_m + To, adam_v + To,
                       (const float *)&st->actor_step_size, (const float *)&st->entropy_step_size, F.learn_entropy, h->beta1, h->beta2,
                       h->eps);
    return launched("sac_adam_kernel launch: %s");
}

int rover_sac_polyak(const rover_policy_desc *actor, const rover_policy_desc *critic, const rover_sac_hparams *h, float *target,
                     const float *params, void *stream)
{
    if (int rc = check_nets(actor, critic)) return rc;
    if (!h || !target || !params) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    int dev;
    if (int rc = device_of(target, &dev)) return rc;
    DeviceGuard guard(dev);
    const size_t count = 2 * net_floats(true);
    const float keep = (float)(1.0 - (double)h->polyak);
    hipLaunchKernelGGL(sac_polyak_kernel, dim3((unsigned)((count + FT - 1) / FT)), dim3(FT), 0, static_cast<hipStream_t>(stream), target,
                       params + net_floats(false), count, keep, h->polyak);
    return launched("sac_polyak_kernel launch: %s");
}

}  // extern "C"
