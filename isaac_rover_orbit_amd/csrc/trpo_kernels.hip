// trpo_kernels.hip -- fused TRPO update of the rover's policy / value networks (gfx950 / CDNA4, wave64).
//
// skrl TRPO._update for the reference architecture; see include/rover_trpo.h for the contract and the reduction order.
// The networks run layer by layer over all rows, every dense product on v_mfma_f32_16x16x4_f32:
//   trpo_dense_kernel    forward Z = A W^T + b, act(Z); or the forward-mode JVP dZ = dA W^T + A V^T + vb, act'(a) dZ.
//                        One wave per 16 rows x 64 columns; the packed weights are the B fragments as they lie (one float4
//                        per lane per 16 k);
//   trpo_back_kernel     reverse dA = dZ W, times LeakyReLU' of the stored activation; one wave per 16 rows x 64 columns;
//   trpo_wgrad_kernel    dW = dZ^T A and db = sum dZ per (16 x 16 tile, 2048-row chunk), written in the packed layout;
//   trpo_combine_kernel  the chunk partials added in chunk order (plus damping v for a Fisher-vector product);
// plus one-thread-per-row heads (surrogate gradient, FVP scaling, line-search KL / surrogate, value MSE), fixed-order
// reductions and the small CG / line-search / Adam kernels that read and write the device state.  The value step's clip and Adam
// arithmetic, w_at, the packed sizes and the reference-architecture check are train_shared.hpp's, device_of and launched
// rover_internal.hpp's; the network kernels are this file's own.
//
// The theta_old forward of rover_trpo_policy_grad caches every activation (690 floats per row), so a Fisher-vector product
// is a JVP (6 dense launches), a head, a reverse pass (5 launches) and the weight gradients (1 launch + combine).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_hip.h"
#include "../../include/rover_policy.h"
#include "../../include/rover_trpo.h"
#include "rover_internal.hpp"
#include "train_shared.hpp"

namespace {

constexpr int OBS = 965, PROP = 4, ENC_OFF = 3;
constexpr int NL = 6;
constexpr int LK[NL] = {961, 80, 64, 256, 160, 128};          // in features of the reference layers
constexpr int LN[NL - 1] = {80, 60, 256, 160, 128};          // out features of layers 1 .. 5 (layer 6: 2 policy, 1 value)
constexpr int FT = 256;                                      // threads of every multi-thread kernel here
constexpr int NORM_BLOCKS = 128;                             // fixed chunks of a vector reduction
constexpr int CH = 2048;                                     // rows per weight-gradient chunk
// per-row matrices of a network region (cache = activations at theta_old, scratch = JVP / reverse / trial forward):
// width of the output of layer l (layer 2's output sits at columns 4 .. 63 of the 64-wide MLP input M)
constexpr int MW[NL] = {80, 64, 256, 160, 128, 2};
constexpr int ROW_F = 80 + 64 + 256 + 160 + 128 + 2;        // 690
constexpr int HEAD_F = 1024;                                 // reduction partials at the start of the workspace

struct Nets {
    uint32_t net_off[2];          // start of the policy / value packed block
    uint32_t w_off[2][NL], b_off[2][NL];
    uint32_t ls_off;              // log_std
    uint32_t net_floats[2];
    float slope;
};

__device__ __forceinline__ bool skipped(const int32_t *w) { return w && *(volatile const int32_t *)w != 0; }
__device__ __forceinline__ float clamp_ls(float s, float lo, float hi) { return fminf(fmaxf(s, lo), hi); }
__device__ __forceinline__ float in_clamp(float s, float lo, float hi) { return (s >= lo && s <= hi) ? 1.0f : 0.0f; }

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

// ---- dense layer: forward or JVP
enum { ACT_NONE_ = 0, ACT_LEAKY_ = 1, ACT_TANH_ = 2 };
struct DenseArgs {
    const float *x; int xp;        // input A (row r, column k at x[row(r) * xp + k])
    const int64_t *idx;            // x rows gathered by idx (layer 1 of a minibatch) or NULL
    const float *dx; int dxp;      // JVP: dA of the input (NULL: the input does not depend on theta)
    const float *W, *b;            // packed weights / bias (theta for a forward, theta_old for a JVP)
    const float *V, *vb;           // JVP: the direction's packed weights / bias; NULL: forward
    const float *aref; int arp;    // JVP: the stored output activation of this layer (act')
    float *out; int op, ocol;      // output matrix, pitch, first column
    const float *prop;             // forward of layer 2: out[r][0 .. 4) = prop row (the obs, gathered by pidx); JVP: zeros
    const int64_t *pidx;
    int K, N, rows, act;
    float slope;
    const int32_t *skip;
};

__global__ __launch_bounds__(FT) void trpo_dense_kernel(DenseArgs A)
{
    if (skipped(A.skip)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rr = lane >> 4, cc = lane & 15;
    const int r0 = blockIdx.x * 64 + wave * 16, t0 = blockIdx.y * 4;    // first row, first 16-column tile
    const int G = cdiv(A.K, 16), NT = cdiv(A.N, 16);
    if (A.prop && blockIdx.y == 0 && lane < 64) {                        // the proprioceptive columns of M
        const int r = r0 + (lane >> 2), c = lane & 3;
        if (r < A.rows) {
            const size_t src = A.pidx ? (size_t)A.pidx[r] : (size_t)r;
            A.out[(size_t)r * A.op + c] = A.V ? 0.0f : A.prop[src * OBS + c];
        }
    }
    const int ra = r0 + cc;                                              // the A operand's row of this lane
    const bool row_ok = ra < A.rows;
    const float *xrow = row_ok ? A.x + (A.idx ? (size_t)A.idx[ra] : (size_t)ra) * A.xp : A.x;
    const float *dxrow = (row_ok && A.dx) ? A.dx + (size_t)ra * A.dxp : nullptr;
    v4f acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    // sum_k a[r][k] * M[n][k] with M's packed fragments: lane (n & 15) + 16 (k & 3) of fragment (n / 16, k / 16) holds
    // M[n][16 g + 4 e + (k & 3)] in element e, exactly the B operand (k = rr, j = cc) of the 4 MFMAs of a 16-k group
    auto gemm = [&](const float *arow, const float *M) __attribute__((always_inline)) {
        for (int g = 0; g < G; ++g) {
            float a[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 16 * g + 4 * e + rr;
                a[e] = (arow && k < A.K) ? arow[k] : 0.0f;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t0 + t < NT) {
                    const v4f w = reinterpret_cast<const v4f *>(M)[((size_t)(t0 + t) * G + g) * 64 + cc + 16 * rr];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], w[e], acc[t], 0, 0, 0);
                }
            }
        }
    };
    if (A.V) {
        if (A.dx) gemm(dxrow, A.W);
        gemm(row_ok ? xrow : nullptr, A.V);
    } else {
        gemm(row_ok ? xrow : nullptr, A.W);
    }
    // D[i][j]: lane holds i = 4 rr + jj, j = cc
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = 16 * (t0 + t) + cc;
        if (t0 + t >= NT || col >= A.N) continue;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int r = r0 + 4 * rr + jj;
            if (r >= A.rows) continue;
            float z;
            if (A.V) {
                const float d = acc[t][jj] + A.vb[col];
                const float a = A.aref[(size_t)r * A.arp + A.ocol + col];
                z = A.act == ACT_LEAKY_ ? (a > 0.0f ? d : d * A.slope) : A.act == ACT_TANH_ ? d * (1.0f - a * a) : d;
            } else {
                const float s = acc[t][jj] + A.b[col];
                z = A.act == ACT_LEAKY_ ? (s > 0.0f ? s : s * A.slope) : A.act == ACT_TANH_ ? tanhf(s) : s;
            }
            A.out[(size_t)r * A.op + A.ocol + col] = z;
        }
    }
}

// ---- reverse: dZ_prev[r][k] = (sum_n dZ[r][n] W[n][k]) * LeakyReLU'(a_prev[r][k]) for k in [k0, k0 + nk)
struct BackArgs {
    const float *dz; int dzp;      // dZ of layer l (rows, N)
    const float *W; int K, N;      // packed weights of layer l (N x K)
    const float *aref; int arp;    // stored input activation of layer l
    float *out; int op;            // dZ of layer l - 1, column k at out[r * op + k]
    int k0, nk, rows;
    float slope;
    const int32_t *skip;
};
__global__ __launch_bounds__(FT) void trpo_back_kernel(BackArgs A)
{
    if (skipped(A.skip)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rr = lane >> 4, cc = lane & 15;
    const int r0 = blockIdx.x * 64 + wave * 16, c0 = blockIdx.y * 64;    // first row, first output column (relative to k0)
    const int G = cdiv(A.K, 16);
    const int ra = r0 + cc;
    const bool row_ok = ra < A.rows;
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
            if (r >= A.rows) continue;
            const float d = acc[t][jj];
            A.out[(size_t)r * A.op + k] = A.aref[(size_t)r * A.arp + k] > 0.0f ? d : d * A.slope;
        }
    }
}

// ---- weight / bias gradients: one wave per (layer, 16 x 16 tile of the packed weights or a 16-row bias tile, chunk)
struct WgradArgs {
    const float *obs; const int64_t *idx;     // layer 1's input
    const float *am[NL]; int ap[NL];          // input activation of layer l (l >= 1), pitch
    const float *dz[NL]; int dzp[NL];         // dZ of layer l, pitch
    int K[NL], N[NL];
    uint32_t w_off[NL], b_off[NL];
    int jobs[NL + 1];                         // prefix sums of the per-layer job counts
    int rows, P;                              // rows; packed floats of the network (the partial's stride)
    float *part;                              // (chunks, P)
    const int32_t *skip;
};
__global__ __launch_bounds__(FT) void trpo_wgrad_kernel(WgradArgs A)
{
    if (skipped(A.skip)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int job = blockIdx.x * 4 + wave;
    if (job >= A.jobs[NL]) return;
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
    const float *dz = A.dz[l];
    const int dzp = A.dzp[l];
    v4f acc = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    // A operand: lane (i = cc, k = rr) = dZ[row][16 t + cc]; B operand: lane (k = rr, j = cc) = A[row][16 g + cc]
    for (int rb = rb0; rb < rb1; rb += 4) {
        const int r = rb + rr;
        const bool ok = r < rb1;
        const float a = ok && col_ok ? dz[(size_t)r * dzp + col] : 0.0f;
        float b;
        if (bias) b = ok ? 1.0f : 0.0f;
        else if (l == 0) b = ok && k_ok ? A.obs[(A.idx ? (size_t)A.idx[r] : (size_t)r) * OBS + ENC_OFF + kin] : 0.0f;
        else b = ok && k_ok ? A.am[l][(size_t)r * A.ap[l] + kin] : 0.0f;
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

// out[off + e] = sum_c part[c][e] (c ascending) + damping v[off + e] for e < P; with `zero_len` > 0 also writes zeros to
// out[zero_off .. zero_off + zero_len) (the other network's block of a policy-side vector)
__global__ __launch_bounds__(FT) void trpo_combine_kernel(const float *part, int nch, int P, uint32_t off, const float *v, float damping,
                                                          float *out, uint32_t zero_off, int zero_len, const int32_t *skip)
{
    if (skipped(skip)) return;
    const int e = blockIdx.x * FT + threadIdx.x;
    if (e < P) {
        float s = part[e];
        for (int c = 1; c < nch; ++c) s += part[(size_t)c * P + e];
        if (v) s += damping * v[off + e];
        out[off + e] = s;
    }
    if (e < zero_len) out[zero_off + e] = 0.0f;
}

// ---- per-row heads: one thread per row, the block's partial sums (fixed tree) to rowp[block * 4 + i]
struct HeadArgs {
    const float *mu; int mup;          // tanh mean at theta_old (cache)
    float *y; int yp;                  // scratch last layer: JVP output / dZ6 / trial mean / value output
    const float *act, *logp, *adv, *ret;
    const int64_t *idx;
    const float *ls_now, *ls_old;      // raw log_std: of params and of the theta_old copy
    float ls_min, ls_max, inv_n, vscale;
    int rows;
    float *rowp;
    const int32_t *skip;
};
enum { HEAD_GRAD = 0, HEAD_FVP = 1, HEAD_LS = 2, HEAD_VALUE = 3 };
template <int MODE>
__global__ __launch_bounds__(FT) void trpo_head_kernel(HeadArgs A)
{
    __shared__ float red[FT];
    if (skipped(A.skip)) return;
    const int r = blockIdx.x * FT + threadIdx.x;
    float t[3] = {0.0f, 0.0f, 0.0f};
    if (r < A.rows) {
        if (MODE == HEAD_VALUE) {
            const float v = A.mu[(size_t)r * A.mup];                           // the cached value output
            const float err = A.ret[A.idx[r]] - v;
            t[0] = A.vscale * (err * err);
            A.y[(size_t)r * A.yp] = -2.0f * A.vscale * err * A.inv_n;          // d(mse)/dV
        } else {
            float s[2], sg[2];
            for (int i = 0; i < 2; ++i) {
                s[i] = clamp_ls(A.ls_now[i], A.ls_min, A.ls_max);
                sg[i] = expf(s[i]);
            }
            if (MODE == HEAD_FVP) {
                for (int i = 0; i < 2; ++i) {
                    const float mu = A.mu[(size_t)r * A.mup + i];
                    const float u = A.y[(size_t)r * A.yp + i] / (sg[i] * sg[i]) * A.inv_n;     // sigma^-2 J v / B
                    A.y[(size_t)r * A.yp + i] = u * (1.0f - mu * mu);                        // through tanh
                }
            } else {
                const float *mu = MODE == HEAD_GRAD ? A.mu + (size_t)r * A.mup : A.y + (size_t)r * A.yp;
                float x[2], lp = 0.0f;
                for (int i = 0; i < 2; ++i) {
                    x[i] = (A.act[2 * (size_t)r + i] - mu[i]) / sg[i];
                    lp += -0.5f * x[i] * x[i] - s[i] - 0.9189385332f;
                }
                const float ratio = expf(lp - A.logp[r]), w = A.adv[r] * ratio;
                if (MODE == HEAD_GRAD) {
                    t[0] = w;
                    for (int i = 0; i < 2; ++i) {
                        t[1 + i] = w * (x[i] * x[i] - 1.0f);                                 // dL/ds_i * B
                        const float dmu = w * x[i] / sg[i] * A.inv_n;                         // dL/dmu_i
                        A.y[(size_t)r * A.yp + i] = dmu * (1.0f - mu[i] * mu[i]);
                    }
                } else {                                                                      // line search
                    float kl = 0.0f;
                    for (int i = 0; i < 2; ++i) {
                        const float so = clamp_ls(A.ls_old[i], A.ls_min, A.ls_max), sgo = expf(so);
                        const float d = A.mu[(size_t)r * A.mup + i] - mu[i];
                        kl += so - s[i] + 0.5f * (sgo * sgo + d * d) / (sg[i] * sg[i]) - 0.5f;
                    }
                    t[0] = kl;
                    t[1] = w;
                }
            }
        }
    }
    if (MODE == HEAD_FVP) return;
    for (int i = 0; i < 3; ++i) {
        const float tot = block_sum(t[i], red);
        if (threadIdx.x == 0) A.rowp[(size_t)blockIdx.x * 4 + i] = tot;
    }
}

// thread t adds partials t, t + 256, ... in order, then the tree; totals of the 3 row-terms in tot[0 .. 3) (thread 0)
__device__ void reduce_rows(const float *rowp, int nblk, float *tot, float *red)
{
    for (int i = 0; i < 3; ++i) {
        float s = 0.0f;
        for (int b = threadIdx.x; b < nblk; b += FT) s += rowp[(size_t)b * 4 + i];
        tot[i] = block_sum(s, red);
    }
}

__global__ void trpo_reset_kernel(rover_trpo_state *st)
{
    const int32_t vs = st->value_step;
    memset(st, 0, sizeof(*st));
    st->value_step = vs;
    st->accepted = -1;
}

// after HEAD_GRAD: L_old, the log_std gradient and its padding; the value block of grad is zeroed by the combine
__global__ __launch_bounds__(FT) void trpo_grad_final_kernel(const float *rowp, int nblk, float inv_n, const float *params, uint32_t ls_off,
                                                             float ls_min, float ls_max, float *grad, rover_trpo_state *st)
{
    __shared__ float red[FT];
    float tot[3];
    reduce_rows(rowp, nblk, tot, red);
    if (threadIdx.x == 0) {
        st->loss_old = tot[0] * inv_n;
        for (int i = 0; i < 2; ++i) grad[ls_off + i] = in_clamp(params[ls_off + i], ls_min, ls_max) * (tot[1 + i] * inv_n);
        grad[ls_off + 2] = 0.0f;
        grad[ls_off + 3] = 0.0f;
    }
}
// the log_std block of F v: (2 c_i + damping) v_i; padding 0
__global__ void trpo_fvp_ls_kernel(const float *params, const float *v, uint32_t ls_off, float ls_min, float ls_max, float damping,
                                   float *out, const int32_t *skip)
{
    if (skipped(skip)) return;
    const int i = threadIdx.x;
    if (i < 2) out[ls_off + i] = 2.0f * in_clamp(params[ls_off + i], ls_min, ls_max) * v[ls_off + i] + damping * v[ls_off + i];
    else if (i < 4) out[ls_off + i] = 0.0f;
}

// ---- vector kernels over P floats (NORM_BLOCKS fixed chunks)
// part[b] = sum over chunk b of a[e] * c[e]
__global__ __launch_bounds__(FT) void trpo_dot_kernel(const float *a, const float *c, int P, float *part, const int32_t *skip)
{
    __shared__ float red[FT];
    if (skipped(skip)) return;
    const int chunk = cdiv(P, NORM_BLOCKS), e0 = blockIdx.x * chunk, e1 = min(e0 + chunk, P);
    float s = 0.0f;
    for (int e = e0 + threadIdx.x; e < e1; e += FT) s += a[e] * c[e];
    const float tot = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
__device__ float reduce_part(const float *part, float *red) { return block_sum((int)threadIdx.x < NORM_BLOCKS ? part[threadIdx.x] : 0.0f, red); }

// CG start: x = 0, r = p = g, rr_old = g.g (from the dot partials)
__global__ __launch_bounds__(FT) void trpo_cg_init_kernel(const float *g, float *x, float *r, float *p, int P)
{
    const int e = blockIdx.x * FT + threadIdx.x;
    if (e >= P) return;
    x[e] = 0.0f;
    r[e] = g[e];
    p[e] = g[e];
}
__global__ __launch_bounds__(FT) void trpo_cg_rr0_kernel(const float *part, rover_trpo_state *st)
{
    __shared__ float red[FT];
    const float rr = reduce_part(part, red);
    if (threadIdx.x == 0) { st->rr_old = rr; st->rr = rr; }
}
// alpha = rr_old / p.hv
__global__ __launch_bounds__(FT) void trpo_cg_alpha_kernel(const float *part, rover_trpo_state *st)
{
    __shared__ float red[FT];
    if (skipped(&st->cg_done)) return;
    const float php = reduce_part(part, red);
    if (threadIdx.x == 0) st->cg_alpha = st->rr_old / php;
}
// x += alpha p; r -= alpha hv; part[b] = the chunk's sum of r_new^2
__global__ __launch_bounds__(FT) void trpo_cg_xr_kernel(float *x, float *r, const float *p, const float *hv, int P, float *part,
                                                        const rover_trpo_state *st)
{
    __shared__ float red[FT];
    if (skipped(&st->cg_done)) return;
    const float alpha = st->cg_alpha;
    const int chunk = cdiv(P, NORM_BLOCKS), e0 = blockIdx.x * chunk, e1 = min(e0 + chunk, P);
    float s = 0.0f;
    for (int e = e0 + threadIdx.x; e < e1; e += FT) {
        x[e] = x[e] + alpha * p[e];
        const float rn = r[e] - alpha * hv[e];
        r[e] = rn;
        s += rn * rn;
    }
    const float tot = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
// rr_new; stop below the tolerance, else beta = rr_new / rr_old, rr_old = rr_new
__global__ __launch_bounds__(FT) void trpo_cg_beta_kernel(const float *part, float tol, rover_trpo_state *st)
{
    __shared__ float red[FT];
    if (skipped(&st->cg_done)) return;
    const float rr = reduce_part(part, red);
    if (threadIdx.x == 0) {
        st->cg_iters += 1;
        st->rr = rr;
        if (rr < tol) {
            st->cg_done = 1;
        } else {
            st->cg_beta = rr / st->rr_old;
            st->rr_old = rr;
        }
    }
}
__global__ __launch_bounds__(FT) void trpo_cg_p_kernel(float *p, const float *r, int P, const rover_trpo_state *st)
{
    if (skipped(&st->cg_done)) return;
    const int e = blockIdx.x * FT + threadIdx.x;
    if (e >= P) return;
    p[e] = r[e] + st->cg_beta * p[e];
}

// step = sqrt(2 max_kl / xHx) from the x.hv partials
__global__ __launch_bounds__(FT) void trpo_step_kernel(const float *part, float max_kl, rover_trpo_state *st)
{
    __shared__ float red[FT];
    const float xhx = reduce_part(part, red);
    if (threadIdx.x == 0) {
        st->xhx = xhx;
        st->step = sqrtf((2.0f * max_kl) / xhx);
    }
}
__global__ __launch_bounds__(FT) void trpo_full_kernel(const float *x, float *full, int P, const rover_trpo_state *st)
{
    const int e = blockIdx.x * FT + threadIdx.x;
    if (e < P) full[e] = st->step * x[e];
}
__global__ __launch_bounds__(FT) void trpo_expected_kernel(const float *part, rover_trpo_state *st)
{
    __shared__ float red[FT];
    const float ex = reduce_part(part, red);
    if (threadIdx.x == 0) st->expected = ex;
}

// ---- line search
// theta = theta_old + alpha full over the policy block and log_std; E *= alpha
__global__ __launch_bounds__(FT) void trpo_trial_kernel(float *params, const float *old, const float *full, float alpha, uint32_t Pp,
                                                        uint32_t ls_off, int trial, rover_trpo_state *st)
{
    if (skipped(&st->ls_done)) return;
    const uint32_t e = blockIdx.x * FT + threadIdx.x;
    uint32_t at;
    if (e < Pp) at = e;
    else if (e < Pp + 2) at = ls_off + (e - Pp);
    else {
        if (e == Pp + 2) { st->expected = st->expected * alpha; st->trials = trial + 1; }
        return;
    }
    params[at] = old[at] + alpha * full[at];
}
__global__ __launch_bounds__(FT) void trpo_accept_kernel(const float *rowp, int nblk, float inv_n, float max_kl, float accept_ratio,
                                                         int trial, rover_trpo_state *st)
{
    __shared__ float red[FT];
    if (skipped(&st->ls_done)) return;
    float tot[3];
    reduce_rows(rowp, nblk, tot, red);
    if (threadIdx.x == 0) {
        const float kl = tot[0] * inv_n, loss = tot[1] * inv_n;
        st->kl = kl;
        st->loss_new = loss;
        if (kl < max_kl && (loss - st->loss_old) / st->expected > accept_ratio) {
            st->ls_done = 1;
            st->accepted = trial;
        }
    }
}
// no trial accepted: theta_old back, bit for bit; then the replicas of the policy block
__global__ __launch_bounds__(FT) void trpo_restore_kernel(float *params, const float *old, uint32_t Pp, uint32_t ls_off, float *rep, int n_copies,
                                                          const rover_trpo_state *st)
{
    const uint32_t e = blockIdx.x * FT + threadIdx.x;
    const bool restore = *(volatile const int32_t *)&st->ls_done == 0;
    if (e < Pp) {
        const float p = restore ? old[e] : params[e];
        params[e] = p;
        if (rep)
            for (int c = 0; c < n_copies; ++c) rep[(size_t)c * Pp + e] = p;
    } else if (e < Pp + 2 && restore) {
        params[ls_off + (e - Pp)] = old[ls_off + (e - Pp)];
    }
}

// ---- value minibatch loss and clip + Adam over the value block
__global__ __launch_bounds__(FT) void trpo_value_final_kernel(const float *rowp, int nblk, float inv_n, rover_trpo_state *st)
{
    __shared__ float red[FT];
    float tot[3];
    reduce_rows(rowp, nblk, tot, red);
    if (threadIdx.x == 0) {
        st->value_loss_sum += tot[0] * inv_n;
        st->value_batches += 1;
    }
}
__global__ __launch_bounds__(FT) void trpo_adam_prep_kernel(const float *part, float max_norm, float beta1, float beta2, float lr,
                                                            rover_trpo_state *st)
{
    __shared__ float red[FT];
    const float tot = reduce_part(part, red);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(tot);
        st->grad_norm = norm;
        st->clip_coef = grad_clip_coef(norm, max_norm);
        st->value_step += 1;
        adam_scalars(st->value_step, beta1, beta2, lr, &st->step_size, &st->bc2_sqrt);
    }
}
__global__ __launch_bounds__(FT) void trpo_adam_kernel(float *params, float *grad, float *m, float *v, const rover_trpo_state *st, int P,
                                                       float beta1, float beta2, float eps, float *rep, int n_copies)
{
    const int e = blockIdx.x * FT + threadIdx.x;
    if (e >= P) return;
    const float p = adam_element_clipped(params, grad, m, v, e, &st->clip_coef, &st->step_size, &st->bc2_sqrt, beta1, beta2, eps);
    refresh_replicas(rep, n_copies, P, e, p);
}

// ---- host side
size_t ref_net_floats(int nout)
{
    size_t n = 0;
    for (int l = 0; l < NL; ++l) {
        const int N = l < NL - 1 ? LN[l] : nout;
        n += layer_weight_floats(N, LK[l]) + layer_bias_floats(N);
    }
    return n;
}
size_t ref_param_floats() { return ref_net_floats(2) + ref_net_floats(1) + 4; }

int check_pair(const rover_policy_desc *pa, const rover_policy_desc *pb)
{
    if (!pa || !pb) return rover_internal_fail(ROVER_ERR_INVALID, "descriptor is NULL");
    if (!is_reference(pa, 2, ROVER_ACT_TANH) || !is_reference(pb, 1, ROVER_ACT_NONE))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "the fused TRPO update runs the reference architecture only (policy: "
                                                          "rover_policy_default_desc(2, 1), value: (1, 0), packed by rover_policy_pack)");
    return ROVER_OK;
}
Nets nets_of(const rover_policy_desc *pa, const rover_policy_desc *pb)
{
    Nets s;
    const rover_policy_desc *d[2] = {pa, pb};
    s.net_floats[0] = (uint32_t)ref_net_floats(2);
    s.net_floats[1] = (uint32_t)ref_net_floats(1);
    s.net_off[0] = 0;
    s.net_off[1] = s.net_floats[0];
    s.ls_off = s.net_floats[0] + s.net_floats[1];
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < NL; ++i) { s.w_off[k][i] = d[k]->layers[i].w_off; s.b_off[k][i] = d[k]->layers[i].b_off; }
    s.slope = pa->leaky_slope;
    return s;
}

// workspace layout (floats): HEAD_F reduction partials; policy region for `rows` rows: vectors g, x, r, p, hv, full, theta_old
// (P each), cache and scratch (ROW_F per row), row partials, chunk partials; then the value region for `mb` rows
struct Region {
    float *cache[NL], *scr[NL];      // per-layer matrices (output of layer l), pitch MW[l]
    float *rowp, *part;
    int rows;
};
size_t region_floats(int rows, size_t Pnet)
{
    return 2 * (size_t)ROW_F * rows + al4(4 * (size_t)cdiv(rows, FT)) + (size_t)cdiv(rows, CH) * Pnet;
}
size_t vec_floats() { return al4(ref_param_floats()); }
size_t ws_floats(int rows, int mb)
{
    return HEAD_F + 7 * vec_floats() + region_floats(rows, ref_net_floats(2)) + region_floats(mb, ref_net_floats(1));
}
Region region_at(float *base, int rows, size_t Pnet)
{
    Region g;
    float *c = base, *s = base + (size_t)ROW_F * rows;
    for (int l = 0; l < NL; ++l) {
        g.cache[l] = c; g.scr[l] = s;
        c += (size_t)MW[l] * rows; s += (size_t)MW[l] * rows;
    }
    g.rowp = base + 2 * (size_t)ROW_F * rows;
    g.part = g.rowp + al4(4 * (size_t)cdiv(rows, FT));
    g.rows = rows;
    (void)Pnet;
    return g;
}
struct Ws {
    float *head;
    float *g, *x, *r, *p, *hv, *full, *old;
    Region pol, val;
};
// the rows the workspace was sized for are not recorded in it: the policy region needs B, the value region (rows, mb)
Ws ws_at(void *ws, int rows, int mb)
{
    Ws w;
    float *f = static_cast<float *>(ws);
    w.head = f;
    float *v = f + HEAD_F;
    const size_t V = vec_floats();
    w.g = v; w.x = v + V; w.r = v + 2 * V; w.p = v + 3 * V; w.hv = v + 4 * V; w.full = v + 5 * V; w.old = v + 6 * V;
    float *pol = v + 7 * V;
    w.pol = region_at(pol, rows, ref_net_floats(2));
    if (mb > 0) w.val = region_at(pol + region_floats(rows, ref_net_floats(2)), mb, ref_net_floats(1));
    return w;
}

// one network's forward over a region's rows: layer outputs into `dst` (cache or scratch)
int forward(const Nets &nets, int net, const float *params, const float *obs, const int64_t *idx, Region &R, float *const *dst,
            const int32_t *skip, hipStream_t s)
{
    const float *base = params + nets.net_off[net];
    for (int l = 0; l < NL; ++l) {
        DenseArgs A = {};
        const int N = l < NL - 1 ? LN[l] : (net == 0 ? 2 : 1);
        if (l == 0) { A.x = obs + ENC_OFF; A.xp = OBS; A.idx = idx; }
        else { A.x = dst[l - 1]; A.xp = MW[l - 1]; }
        A.W = base + nets.w_off[net][l]; A.b = base + nets.b_off[net][l];
        A.out = dst[l]; A.op = MW[l]; A.ocol = l == 1 ? PROP : 0;
        A.prop = l == 1 ? obs : nullptr;
        A.pidx = idx;
        A.K = LK[l]; A.N = N; A.rows = R.rows;
        A.act = l < NL - 1 ? ACT_LEAKY_ : (net == 0 ? ACT_TANH_ : ACT_NONE_);
        A.slope = nets.slope; A.skip = skip;
        hipLaunchKernelGGL(trpo_dense_kernel, dim3(cdiv(R.rows, 64), cdiv(N, 64)), dim3(FT), 0, s, A);
        if (int rc = launched("trpo_dense_kernel launch: %s")) return rc;
    }
    return ROVER_OK;
}

// reverse pass from dZ6 in scr[5] down to dZ1 in scr[0], then the weight gradients into `out` (+ damping v)
int backward_wgrad(const Nets &nets, int net, const float *params, const float *obs, const int64_t *idx, Region &R, const float *v,
                   float damping, float *out, uint32_t zero_off, int zero_len, const int32_t *skip, hipStream_t s)
{
    const float *base = params + nets.net_off[net];
    const int nout = net == 0 ? 2 : 1;
    // layer l's backward: dZ_{l-1} = (dZ_l W_l) * act'(a_{l-1}), a_{l-1} = cache[l - 1]
    for (int l = NL - 1; l >= 1; --l) {
        BackArgs B = {};
        B.dz = l == 1 ? R.scr[1] + PROP : R.scr[l]; B.dzp = MW[l];
        B.W = base + nets.w_off[net][l]; B.K = LK[l]; B.N = l < NL - 1 ? LN[l] : nout;
        B.aref = R.cache[l - 1]; B.arp = MW[l - 1];
        B.out = R.scr[l - 1]; B.op = MW[l - 1];
        B.k0 = l == 2 ? PROP : 0; B.nk = l == 2 ? LN[1] : LK[l];
        B.rows = R.rows; B.slope = nets.slope; B.skip = skip;
        hipLaunchKernelGGL(trpo_back_kernel, dim3(cdiv(R.rows, 64), cdiv(B.nk, 64)), dim3(FT), 0, s, B);
        if (int rc = launched("trpo_back_kernel launch: %s")) return rc;
    }
    WgradArgs W = {};
    W.obs = obs; W.idx = idx;
    W.jobs[0] = 0;
    for (int l = 0; l < NL; ++l) {
        W.K[l] = LK[l]; W.N[l] = l < NL - 1 ? LN[l] : nout;
        W.am[l] = l > 0 ? R.cache[l - 1] : nullptr; W.ap[l] = l > 0 ? MW[l - 1] : 0;
        // dZ of layer 2 (the encoder's 60 outputs) sits at columns 4 .. 63 of its 64-wide matrix
        W.dz[l] = l == 1 ? R.scr[1] + PROP : R.scr[l]; W.dzp[l] = MW[l];
        W.w_off[l] = nets.w_off[net][l]; W.b_off[l] = nets.b_off[net][l];
        W.jobs[l + 1] = W.jobs[l] + cdiv(W.N[l], 16) * (cdiv(LK[l], 16) + 1);
    }
    W.rows = R.rows; W.P = (int)nets.net_floats[net]; W.part = R.part; W.skip = skip;
    const int nch = cdiv(R.rows, CH);
    hipLaunchKernelGGL(trpo_wgrad_kernel, dim3(cdiv(W.jobs[NL], 4), nch), dim3(FT), 0, s, W);
    if (int rc = launched("trpo_wgrad_kernel launch: %s")) return rc;
    const int P = W.P, n = P > zero_len ? P : zero_len;
    hipLaunchKernelGGL(trpo_combine_kernel, dim3(cdiv(n, FT)), dim3(FT), 0, s, (const float *)R.part, nch, P, nets.net_off[net], v, damping,
                       out, zero_off, zero_len, skip);
    return launched("trpo_combine_kernel launch: %s");
}

HeadArgs head_args(const Nets &nets, const rover_trpo_hparams *h, const float *params, Region &R, int rows)
{
    HeadArgs H = {};
    H.mu = R.cache[NL - 1]; H.mup = MW[NL - 1];
    H.y = R.scr[NL - 1]; H.yp = MW[NL - 1];
    H.ls_now = params + nets.ls_off;
    H.ls_min = h->log_std_min; H.ls_max = h->log_std_max;
    H.inv_n = 1.0f / (float)rows;
    H.vscale = h->value_loss_scale;
    H.rows = rows;
    H.rowp = R.rowp;
    return H;
}

int fvp_impl(const Nets &nets, const rover_trpo_hparams *h, const float *params, const float *obs, Ws &w, const float *v, float *out,
             const int32_t *skip, hipStream_t s)
{
    Region &R = w.pol;
    const float *base = params;   // the policy block starts at 0
    const float *vb = v;          // the direction's policy block, same layout
    for (int l = 0; l < NL; ++l) {
        DenseArgs A = {};
        const int N = l < NL - 1 ? LN[l] : 2;
        if (l == 0) { A.x = obs + ENC_OFF; A.xp = OBS; }
        else { A.x = R.cache[l - 1]; A.xp = MW[l - 1]; A.dx = R.scr[l - 1]; A.dxp = MW[l - 1]; }
        A.W = base + nets.w_off[0][l]; A.b = base + nets.b_off[0][l];
        A.V = vb + nets.w_off[0][l]; A.vb = vb + nets.b_off[0][l];
        A.aref = R.cache[l]; A.arp = MW[l];
        A.out = R.scr[l]; A.op = MW[l]; A.ocol = l == 1 ? PROP : 0;
        A.prop = l == 1 ? obs : nullptr;
        A.K = LK[l]; A.N = N; A.rows = R.rows;
        A.act = l < NL - 1 ? ACT_LEAKY_ : ACT_TANH_;
        A.slope = nets.slope; A.skip = skip;
        hipLaunchKernelGGL(trpo_dense_kernel, dim3(cdiv(R.rows, 64), cdiv(N, 64)), dim3(FT), 0, s, A);
        if (int rc = launched("trpo_dense_kernel launch: %s")) return rc;
    }
    HeadArgs H = head_args(nets, h, params, R, R.rows);
    H.skip = skip;
    hipLaunchKernelGGL(trpo_head_kernel<HEAD_FVP>, dim3(cdiv(R.rows, FT)), dim3(FT), 0, s, H);
    if (int rc = launched("trpo_head_kernel launch: %s")) return rc;
    if (int rc = backward_wgrad(nets, 0, params, obs, nullptr, R, v, h->damping, out, nets.net_off[1], (int)nets.net_floats[1], skip, s))
        return rc;
    hipLaunchKernelGGL(trpo_fvp_ls_kernel, dim3(1), dim3(64), 0, s, params, v, nets.ls_off, h->log_std_min, h->log_std_max, h->damping, out,
                       skip);
    return launched("trpo_fvp_ls_kernel launch: %s");
}

int grad_impl(const Nets &nets, const rover_trpo_hparams *h, const float *params, const float *obs, const float *act, const float *logp,
              const float *adv, Ws &w, float *grad, rover_trpo_state *st, hipStream_t s)
{
    Region &R = w.pol;
    const int P = (int)(nets.ls_off + 4);
    hipLaunchKernelGGL(trpo_reset_kernel, dim3(1), dim3(1), 0, s, st);
    if (int rc = launched("trpo_reset_kernel launch: %s")) return rc;
    hipError_t e = hipMemcpyAsync(w.old, params, sizeof(float) * P, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "theta_old copy: %s", hipGetErrorString(e));
    if (int rc = forward(nets, 0, params, obs, nullptr, R, R.cache, nullptr, s)) return rc;
    HeadArgs H = head_args(nets, h, params, R, R.rows);
    H.act = act; H.logp = logp; H.adv = adv;
    hipLaunchKernelGGL(trpo_head_kernel<HEAD_GRAD>, dim3(cdiv(R.rows, FT)), dim3(FT), 0, s, H);
    if (int rc = launched("trpo_head_kernel launch: %s")) return rc;
    if (int rc = backward_wgrad(nets, 0, params, obs, nullptr, R, nullptr, 0.0f, grad, nets.net_off[1], (int)nets.net_floats[1], nullptr, s))
        return rc;
    hipLaunchKernelGGL(trpo_grad_final_kernel, dim3(1), dim3(FT), 0, s, (const float *)R.rowp, cdiv(R.rows, FT), H.inv_n, params, nets.ls_off,
                       h->log_std_min, h->log_std_max, grad, st);
    return launched("trpo_grad_final_kernel launch: %s");
}

int common_checks(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_trpo_hparams *h, const void *params,
                  const void *ws, int *dev)
{
    if (int rc = check_pair(policy, value)) return rc;
    if (!h || !params || !ws) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(params)) & 15)
        return rover_internal_fail(ROVER_ERR_INVALID, "workspace and parameters must be 16-byte aligned");
    return device_of(params, dev);
}

}  // namespace

extern "C" {

int rover_trpo_default_hparams(rover_trpo_hparams *h)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "hparams is NULL");
    h->gamma = 0.99f; h->lam = 0.95f;
    h->value_loss_scale = 1.0f;
    h->log_std_min = -20.0f; h->log_std_max = 2.0f;
    h->max_grad_norm = 0.5f;
    h->beta1 = 0.9f; h->beta2 = 0.999f; h->eps = 1e-8f;
    h->value_lr = 1e-3f;
    h->damping = 0.1f; h->max_kl = 0.01f; h->cg_tol = 1e-10f; h->accept_ratio = 0.5f; h->step_fraction = 1.0f;
    h->cg_steps = 10; h->max_backtrack = 10;
    return ROVER_OK;
}
size_t rover_trpo_hparams_bytes(void) { return sizeof(rover_trpo_hparams); }
size_t rover_trpo_state_bytes(void) { return sizeof(rover_trpo_state); }

size_t rover_trpo_param_floats(const rover_policy_desc *policy, const rover_policy_desc *value)
{
    if (!is_reference(policy, 2, ROVER_ACT_TANH) || !is_reference(value, 1, ROVER_ACT_NONE)) return 0;
    return ref_param_floats();
}
size_t rover_trpo_workspace_bytes(int32_t rows, int32_t max_minibatch_rows)
{
    return rows > 0 && max_minibatch_rows > 0 ? sizeof(float) * ws_floats(rows, max_minibatch_rows) : 0;
}

int rover_trpo_policy_grad(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_trpo_hparams *h,
                           const float *params, const float *obs, const float *act, const float *logp, const float *adv,
                           int32_t B, void *ws, size_t ws_bytes, float *grad, void *state, void *stream)
{
    int dev;
    if (int rc = common_checks(policy, value, h, params, ws, &dev)) return rc;
    if (!obs || !act || !logp || !adv || !grad || !state) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (B < 1) return rover_internal_fail(ROVER_ERR_INVALID, "B must be >= 1");
    if (ws_bytes < rover_trpo_workspace_bytes(B, 1)) return rover_internal_fail(ROVER_ERR_INVALID, "TRPO workspace too small");
    if (reinterpret_cast<uintptr_t>(state) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "state must be 8-byte aligned");
    DeviceGuard guard(dev);
    const Nets nets = nets_of(policy, value);
    Ws w = ws_at(ws, B, 0);
    return grad_impl(nets, h, params, obs, act, logp, adv, w, grad, static_cast<rover_trpo_state *>(state), static_cast<hipStream_t>(stream));
}

int rover_trpo_fvp(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_trpo_hparams *h,
                   const float *params, const float *obs, int32_t B, void *ws, size_t ws_bytes, const float *v, float *out,
                   void *stream)
{
    int dev;
    if (int rc = common_checks(policy, value, h, params, ws, &dev)) return rc;
    if (!obs || !v || !out) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (B < 1) return rover_internal_fail(ROVER_ERR_INVALID, "B must be >= 1");
    if (ws_bytes < rover_trpo_workspace_bytes(B, 1)) return rover_internal_fail(ROVER_ERR_INVALID, "TRPO workspace too small");
    DeviceGuard guard(dev);
    const Nets nets = nets_of(policy, value);
    Ws w = ws_at(ws, B, 0);
    return fvp_impl(nets, h, params, obs, w, v, out, nullptr, static_cast<hipStream_t>(stream));
}

int rover_trpo_policy_step(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_trpo_hparams *h,
                           float *params, const float *obs, const float *act, const float *logp, const float *adv, int32_t B,
                           void *ws, size_t ws_bytes, void *state, float *replicas_policy, int32_t n_copies, float *grad_out,
                           float *dir_out, void *stream)
{
    int dev;
    if (int rc = common_checks(policy, value, h, params, ws, &dev)) return rc;
    if (!obs || !act || !logp || !adv || !state) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (B < 1) return rover_internal_fail(ROVER_ERR_INVALID, "B must be >= 1");
    if (replicas_policy && n_copies < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n_copies must be >= 1");
    if (h->cg_steps < 0 || h->max_backtrack < 0) return rover_internal_fail(ROVER_ERR_INVALID, "cg_steps / max_backtrack must be >= 0");
    if (ws_bytes < rover_trpo_workspace_bytes(B, 1)) return rover_internal_fail(ROVER_ERR_INVALID, "TRPO workspace too small");
    if (reinterpret_cast<uintptr_t>(state) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "state must be 8-byte aligned");
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Nets nets = nets_of(policy, value);
    Ws w = ws_at(ws, B, 0);
    rover_trpo_state *st = static_cast<rover_trpo_state *>(state);
    const int P = (int)(nets.ls_off + 4), nb = cdiv(P, FT);
    float *dotp = w.head;
    if (int rc = grad_impl(nets, h, params, obs, act, logp, adv, w, w.g, st, s)) return rc;
    // ---- CG (skrl conjugate_gradient)
    hipLaunchKernelGGL(trpo_cg_init_kernel, dim3(nb), dim3(FT), 0, s, (const float *)w.g, w.x, w.r, w.p, P);
    hipLaunchKernelGGL(trpo_dot_kernel, dim3(NORM_BLOCKS), dim3(FT), 0, s, (const float *)w.r, (const float *)w.r, P, dotp, nullptr);
    hipLaunchKernelGGL(trpo_cg_rr0_kernel, dim3(1), dim3(FT), 0, s, (const float *)dotp, st);
    if (int rc = launched("trpo CG start launch: %s")) return rc;
    for (int it = 0; it < h->cg_steps; ++it) {
        if (int rc = fvp_impl(nets, h, params, obs, w, w.p, w.hv, &st->cg_done, s)) return rc;
        hipLaunchKernelGGL(trpo_dot_kernel, dim3(NORM_BLOCKS), dim3(FT), 0, s, (const float *)w.p, (const float *)w.hv, P, dotp, &st->cg_done);
        hipLaunchKernelGGL(trpo_cg_alpha_kernel, dim3(1), dim3(FT), 0, s, (const float *)dotp, st);
        hipLaunchKernelGGL(trpo_cg_xr_kernel, dim3(NORM_BLOCKS), dim3(FT), 0, s, w.x, w.r, (const float *)w.p, (const float *)w.hv, P, dotp,
                           (const rover_trpo_state *)st);
        hipLaunchKernelGGL(trpo_cg_beta_kernel, dim3(1), dim3(FT), 0, s, (const float *)dotp, h->cg_tol, st);
        hipLaunchKernelGGL(trpo_cg_p_kernel, dim3(nb), dim3(FT), 0, s, w.p, (const float *)w.r, P, (const rover_trpo_state *)st);
        if (int rc = launched("trpo CG iteration launch: %s")) return rc;
    }
    // ---- step: xHx, step size, full step, expected improvement
    if (int rc = fvp_impl(nets, h, params, obs, w, w.x, w.hv, nullptr, s)) return rc;
    hipLaunchKernelGGL(trpo_dot_kernel, dim3(NORM_BLOCKS), dim3(FT), 0, s, (const float *)w.x, (const float *)w.hv, P, dotp, nullptr);
    hipLaunchKernelGGL(trpo_step_kernel, dim3(1), dim3(FT), 0, s, (const float *)dotp, h->max_kl, st);
    hipLaunchKernelGGL(trpo_full_kernel, dim3(nb), dim3(FT), 0, s, (const float *)w.x, w.full, P, (const rover_trpo_state *)st);
    hipLaunchKernelGGL(trpo_dot_kernel, dim3(NORM_BLOCKS), dim3(FT), 0, s, (const float *)w.g, (const float *)w.full, P, dotp, nullptr);
    hipLaunchKernelGGL(trpo_expected_kernel, dim3(1), dim3(FT), 0, s, (const float *)dotp, st);
    if (int rc = launched("trpo step launch: %s")) return rc;
    for (int k = 0; k < 2; ++k) {
        float *dst = k ? dir_out : grad_out;
        if (!dst) continue;
        hipError_t e = hipMemcpyAsync(dst, k ? w.x : w.g, sizeof(float) * P, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "gradient / direction copy: %s", hipGetErrorString(e));
    }
    // ---- backtracking line search
    Region &R = w.pol;
    const uint32_t Pp = nets.net_floats[0];
    for (int i = 0; i < h->max_backtrack; ++i) {
        const float alpha = (float)((double)h->step_fraction * std::pow(0.5, (double)i));
        hipLaunchKernelGGL(trpo_trial_kernel, dim3(cdiv((int)Pp + 3, FT)), dim3(FT), 0, s, params, (const float *)w.old, (const float *)w.full,
                           alpha, Pp, nets.ls_off, i, st);
        if (int rc = forward(nets, 0, params, obs, nullptr, R, R.scr, &st->ls_done, s)) return rc;
        HeadArgs H = head_args(nets, h, params, R, B);
        H.act = act; H.logp = logp; H.adv = adv; H.ls_old = w.old + nets.ls_off; H.skip = &st->ls_done;
        hipLaunchKernelGGL(trpo_head_kernel<HEAD_LS>, dim3(cdiv(B, FT)), dim3(FT), 0, s, H);
        hipLaunchKernelGGL(trpo_accept_kernel, dim3(1), dim3(FT), 0, s, (const float *)R.rowp, cdiv(B, FT), H.inv_n, h->max_kl, h->accept_ratio,
                           i, st);
        if (int rc = launched("trpo line-search launch: %s")) return rc;
    }
    hipLaunchKernelGGL(trpo_restore_kernel, dim3(cdiv((int)Pp + 2, FT)), dim3(FT), 0, s, params, (const float *)w.old, Pp, nets.ls_off,
                       replicas_policy, (int)n_copies, (const rover_trpo_state *)st);
    return launched("trpo_restore_kernel launch: %s");
}

int rover_trpo_value_minibatch(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_trpo_hparams *h,
                               const float *params, const float *obs, const float *ret, const int64_t *idx, int32_t n,
                               int32_t rows, void *ws, size_t ws_bytes, float *grad, void *state, void *stream)
{
    int dev;
    if (int rc = common_checks(policy, value, h, params, ws, &dev)) return rc;
    if (!obs || !ret || !idx || !grad || !state) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (n < 1 || rows < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n and rows must be >= 1");
    if (ws_bytes < rover_trpo_workspace_bytes(rows, n)) return rover_internal_fail(ROVER_ERR_INVALID, "TRPO workspace too small");
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Nets nets = nets_of(policy, value);
    Ws w = ws_at(ws, rows, n);
    Region &R = w.val;
    if (int rc = forward(nets, 1, params, obs, idx, R, R.cache, nullptr, s)) return rc;
    HeadArgs H = head_args(nets, h, params, R, n);
    H.ret = ret; H.idx = idx;
    hipLaunchKernelGGL(trpo_head_kernel<HEAD_VALUE>, dim3(cdiv(n, FT)), dim3(FT), 0, s, H);
    if (int rc = launched("trpo_head_kernel launch: %s")) return rc;
    if (int rc = backward_wgrad(nets, 1, params, obs, idx, R, nullptr, 0.0f, grad, 0, 0, nullptr, s)) return rc;
    hipLaunchKernelGGL(trpo_value_final_kernel, dim3(1), dim3(FT), 0, s, (const float *)R.rowp, cdiv(n, FT), H.inv_n,
                       static_cast<rover_trpo_state *>(state));
    return launched("trpo_value_final_kernel launch: %s");
}

int rover_trpo_value_apply(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_trpo_hparams *h,
                           float *params, float *grad, float *adam_m, float *adam_v, void *state, float *replicas_value,
                           int32_t n_copies, void *ws, size_t ws_bytes, void *stream)
{
    int dev;
    if (int rc = common_checks(policy, value, h, params, ws, &dev)) return rc;
    if (!grad || !adam_m || !adam_v || !state) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (replicas_value && n_copies < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n_copies must be >= 1");
    if (ws_bytes < rover_trpo_workspace_bytes(1, 1)) return rover_internal_fail(ROVER_ERR_INVALID, "TRPO workspace too small");
    if (reinterpret_cast<uintptr_t>(state) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "state must be 8-byte aligned");
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Nets nets = nets_of(policy, value);
    const uint32_t off = nets.net_off[1];
    const int Pv = (int)nets.net_floats[1];
    float *part = static_cast<float *>(ws);
    rover_trpo_state *st = static_cast<rover_trpo_state *>(state);
    hipLaunchKernelGGL(trpo_dot_kernel, dim3(NORM_BLOCKS), dim3(FT), 0, s, (const float *)grad + off, (const float *)grad + off, Pv, part,
                       nullptr);
    hipLaunchKernelGGL(trpo_adam_prep_kernel, dim3(1), dim3(FT), 0, s, (const float *)part, h->max_grad_norm, h->beta1, h->beta2,
                       h->value_lr, st);
    hipLaunchKernelGGL(trpo_adam_kernel, dim3(cdiv(Pv, FT)), dim3(FT), 0, s, params + off, grad + off, adam_m + off, adam_v + off,
                       (const rover_trpo_state *)st, Pv, h->beta1, h->beta2, h->eps, replicas_value, (int)n_copies);
    return launched("trpo value apply launch: %s");
}

}  // extern "C"
