// lift_ppo_kernels.hip -- fused PPO update of the lift task's policy / value networks (gfx950 / CDNA4, wave64).
//
// Replaces the torch autograd update of isaac_rover_orbit_amd/lift_ppo.py (TorchLiftPPO: skrl 1.1.0 PPO with the lift task's
// skrl_ppo_cfg.yaml) for rover_lift_policy_desc's networks.  See include/rover_lift_train.h for the contract and the reduction
// order.  Kernels, per minibatch:
//   lift_scaler_stats_kernel / lift_scaler_merge_kernel   (first epoch only) the state scaler's update with the gathered raw rows;
//   lift_rows_kernel     one 512-thread workgroup per 16 gathered rows: standardise, forward of both networks on
//                        v_mfma_f32_16x16x4_f32 with rover_policy_forward's exact MFMA sequence, the closed-form loss gradient,
//                        and the backward dA = dZ W on the same MFMA, everything in LDS; stores the standardised rows, the
//                        activations and every dZ for the weight gradients, plus per-workgroup partials;
//   lift_wgrad_kernel    one workgroup per 16 x 16 tile of a weight gradient (or of a bias gradient), dW = dZ^T A on the MFMA
//                        with the rows as k, written in the packed layout;
//   lift_mb_final_kernel one workgroup: log_std gradient, KL and loss terms from the partials; the epoch's early-stop word.
// and per optimiser step lift_sumsq_kernel -> lift_adam_prep_kernel -> lift_adam_kernel (norm, clip, Adam, replica refresh); their
// arithmetic, the KL rate rule and the packed-layout helpers are train_shared.hpp's (the text rover_ppo_apply runs), device_of and
// launched rover_internal.hpp's.
// Every kernel of a minibatch / apply reads the device state first and returns at once while the epoch's stop word is set.
//
// All the lift layers have K and N multiples of 16 except K = 36 of the first layer and the outputs (8, 1), so every product
// runs on the MFMA with zero-fed lanes at the ragged ends (the MI355X guide's exact-f32 MFMA: a k-ordered fmaf chain per 4-k step).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_hip.h"
#include "../../include/rover_lift_train.h"
#include "../../include/rover_policy.h"
#include "rover_internal.hpp"
#include "train_math.hpp"
#include "train_shared.hpp"

namespace {

constexpr int OBS = 36, NACT = 8;
constexpr int NL = 4;
constexpr int LK[NL] = {36, 256, 128, 64};           // in features of the lift layers
constexpr int LN[NL - 1] = {256, 128, 64};           // out features of layers 1 .. 3 (layer 4: 8 policy, 1 value)
constexpr int RB = 16;                               // rows per workgroup of lift_rows_kernel
constexpr int RT = 512;                              // threads of lift_rows_kernel (8 waves)
constexpr int FT = 256;                              // threads of every other multi-thread kernel here
// LDS pitches of the row buffers (columns + 4)
constexpr int PX = 40, P1 = 260, P2 = 132, P3 = 68, P4 = 8;
constexpr int NET_F = RB * (P1 + P2 + P3 + P4);
constexpr int ROWS_LDS_FLOATS = RB * PX + 2 * NET_F + RB * 16;
// workspace: [0, 256) apply partials; [256, 512) scaler batch statistics (2 x 64 doubles); then per network the matrices
// below, each (n, width) row-major; then 16 floats per lift_rows_kernel workgroup
constexpr int WS_HEAD = 512, WS_STATS = 256;
enum { S_X = 0, S_Y1 = 36, S_Y2 = 292, S_Y3 = 420, S_D1 = 484, S_D2 = 740, S_D3 = 868, S_D4 = 932, S_ROW = 940 };
constexpr int PART = 16;
constexpr int NORM_BLOCKS = 128;
constexpr int MAX_SCALER_W = 64;

struct LiftNets {
    uint32_t net_off[2];          // start of the policy / value packed block
    uint32_t w_off[2][NL], b_off[2][NL];
    uint32_t ls_off;              // log_std
    uint32_t net_floats[2];       // packed floats per network (one replica)
    int32_t nout[2];              // 8, 1
};
struct LiftHp {
    float clip, vclip, vscale, ls_min, ls_max, kl_stop, s_eps, s_clip;
};

__device__ __forceinline__ float clampf_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }   // NaN passes
// RunningStandardScaler forward / inverse (rover_lift_train.h), fp32 with explicit roundings
__device__ __forceinline__ float scaler_fwd(float x, double mean, double var, float eps, float clip)
{
    const float d = __fadd_rn(sqrtf((float)var), eps);
    return clampf_nan(__fdiv_rn(__fsub_rn(x, (float)mean), d), -clip, clip);
}
__device__ __forceinline__ float scaler_inv(float x, double mean, double var, float clip)
{
    return __fadd_rn(__fmul_rn(sqrtf((float)var), clampf_nan(x, -clip, clip)), (float)mean);
}

// fixed halving tree over the FT threads of the block; returns the total in every thread
template <typename T>
__device__ __forceinline__ T block_sum(T v, T *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = FT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    const T r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ bool stopped(const rover_lift_ppo_state *st) { return st && *(volatile const int32_t *)&st->stop != 0; }

// ---- RunningStandardScaler: batch statistics per column (one workgroup per column), then the parallel-variance merge
__global__ __launch_bounds__(FT) void lift_scaler_stats_kernel(const float *x, const int64_t *idx, int rows, int width,
                                                               const rover_lift_ppo_state *st, double *bstats)
{
    if (stopped(st)) return;
    __shared__ double red[FT];
    const int c = blockIdx.x;
    auto at = [&](int r) { return (double)x[(size_t)(idx ? idx[r] : r) * width + c]; };
    double s = 0.0;
    for (int r = threadIdx.x; r < rows; r += FT) s += at(r);
    const double mean = block_sum(s, red) / (double)rows;
    double q = 0.0;
    for (int r = threadIdx.x; r < rows; r += FT) {
        const double d = at(r) - mean;
        q += d * d;
    }
    const double m2 = block_sum(q, red);
    if (threadIdx.x == 0) {
        bstats[c] = mean;
        bstats[MAX_SCALER_W + c] = m2 / (double)(rows - 1);   // torch.var: unbiased
    }
}
__global__ void lift_scaler_merge_kernel(double *scaler, int width, int rows, const rover_lift_ppo_state *st, const double *bstats)
{
    if (stopped(st)) return;
    const int c = threadIdx.x;
    double *mean = scaler, *var = scaler + width;
    const double cnt = scaler[2 * width], bc = (double)rows, tot = cnt + bc;
    if (c < width) {
        const double delta = bstats[c] - mean[c];
        const double m2 = var[c] * cnt + bstats[MAX_SCALER_W + c] * bc + delta * delta * cnt * bc / tot;   // skrl _parallel_variance
        mean[c] = mean[c] + delta * bc / tot;
        var[c] = m2 / tot;
    }
    __syncthreads();   // every column has read the old count
    if (c == 0) scaler[2 * width] = tot;
}
__global__ __launch_bounds__(FT) void lift_scaler_apply_kernel(const double *scaler, int width, const float *x, int rows, int inverse,
                                                               float eps, float clip, float *out)
{
    const size_t e = (size_t)blockIdx.x * FT + threadIdx.x;
    if (e >= (size_t)rows * width) return;
    const int c = (int)(e % (size_t)width);
    const double mean = scaler[c], var = scaler[width + c];
    out[e] = inverse ? scaler_inv(x[e], mean, var, clip) : scaler_fwd(x[e], mean, var, eps, clip);
}

// one 16 x 16 output tile of a forward layer: rover_policy_forward's MFMA sequence (k groups ascending, k = 16 g + 4 j + akq)
template <int K>
__device__ __forceinline__ v4f fwd_tile(const float *in, int ip, const v4f *Wt, int arow, int akq)
{
    constexpr int G = (K + 15) / 16;
    v4f b[G];
#pragma unroll
    for (int g = 0; g < G; ++g) b[g] = Wt[(size_t)g * 64];
    v4f acc = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    const float *ap = in + arow * ip + akq;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 16 * g + 4 * j + akq;
            const float a = (K % 16 == 0 || k < K) ? ap[16 * g + 4 * j] : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[g][j], acc, 0, 0, 0);
        }
    return acc;
}

struct RowsArgs {
    LiftNets nets;
    LiftHp hp;
    const float *params, *obs, *act, *logp, *val, *ret, *adv;
    const double *scaler;
    const int64_t *idx;
    const rover_lift_ppo_state *st;
    int n;
    float *ws;          // the matrices (past WS_HEAD)
    float *part;        // PART floats per workgroup
    float *mean_out, *value_out;
};

__global__ __launch_bounds__(RT) void lift_rows_kernel(RowsArgs A)
{
    if (stopped(A.st)) return;
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int arow = lane & 15, akq = lane >> 4;
    const int row0 = blockIdx.x * RB, rows = min(RB, A.n - row0), n = A.n;
    float *X = lds;
    auto y1 = [&](int net) __attribute__((always_inline)) { return lds + RB * PX + net * NET_F; };
    auto y2 = [&](int net) __attribute__((always_inline)) { return y1(net) + RB * P1; };
    auto y3 = [&](int net) __attribute__((always_inline)) { return y2(net) + RB * P2; };
    auto y4 = [&](int net) __attribute__((always_inline)) { return y3(net) + RB * P3; };
    float *rowterm = lds + RB * PX + 2 * NET_F;   // [16][16]
    auto gmat = [&](int net, int slot) __attribute__((always_inline)) { return A.ws + ((size_t)net * S_ROW + slot) * n; };
    auto Wl = [&](int net, int l) __attribute__((always_inline)) { return A.params + A.nets.net_off[net] + A.nets.w_off[net][l]; };
    auto Bl = [&](int net, int l) __attribute__((always_inline)) { return A.params + A.nets.net_off[net] + A.nets.b_off[net][l]; };

    // ---- gather + standardise the rows (state scaler), zero rows past n
    for (int e = tid; e < RB * OBS; e += RT) {
        const int r = e / OBS, c = e - r * OBS;
        float v = 0.0f;
        if (r < rows) {
            v = scaler_fwd(A.obs[(size_t)A.idx[row0 + r] * OBS + c], A.scaler[c], A.scaler[OBS + c], A.hp.s_eps, A.hp.s_clip);
            gmat(0, S_X)[(size_t)(row0 + r) * OBS + c] = v;
        }
        X[r * PX + c] = v;
    }
    __syncthreads();

    // ---- forward, both networks: wave-uniform loop over (network, column tile) items
    auto layer = [&](auto k_tag, int l, auto in_of, int ip, auto out_of, int op, int slot, bool act) __attribute__((always_inline)) {
        constexpr int K = decltype(k_tag)::value;
        const int T = l < NL - 1 ? LN[l] / 16 : 1;
        for (int tt = wave; tt < 2 * T; tt += RT / 64) {
            const int net = tt / T, t = tt - net * T;
            const int N = l < NL - 1 ? LN[l] : A.nets.nout[net];
            const v4f *Wt = reinterpret_cast<const v4f *>(Wl(net, l)) + (size_t)t * ((K + 15) / 16) * 64 + lane;
            const float bv = Bl(net, l)[min(16 * t + arow, N - 1)];
            const v4f acc = fwd_tile<K>(in_of(net), ip, Wt, arow, akq);
            const int col = 16 * t + arow;
            if (col < N) {
                float *dst = out_of(net), *g = slot >= 0 ? gmat(net, slot) : nullptr;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r = 4 * akq + j;
                    const float v = act ? elu(acc[j] + bv) : acc[j] + bv;
                    dst[r * op + col] = v;
                    if (r < rows && slot >= 0) g[(size_t)(row0 + r) * N + col] = v;
                }
            }
        }
        __syncthreads();
    };
    auto xin = [&](int) __attribute__((always_inline)) { return (const float *)X; };
    layer(std::integral_constant<int, 36>{}, 0, xin, PX, y1, P1, S_Y1, true);
    layer(std::integral_constant<int, 256>{}, 1, y1, P1, y2, P2, S_Y2, true);
    layer(std::integral_constant<int, 128>{}, 2, y2, P2, y3, P3, S_Y3, true);
    layer(std::integral_constant<int, 64>{}, 3, y3, P3, y4, P4, -1, false);

    // ---- the loss and dL/d(out) per row (lift_ppo.py lift_ppo_loss), row terms for this workgroup's sums
    if (tid < RB) {
        const int r = tid;
        float t[PART];
#pragma unroll
        for (int i = 0; i < PART; ++i) t[i] = 0.0f;
        float dz[NACT], dzv = 0.0f;
#pragma unroll
        for (int c = 0; c < NACT; ++c) dz[c] = 0.0f;
        if (r < rows) {
            const int64_t row = A.idx[row0 + r];
            const float inv_n = 1.0f / (float)n;
            const float *ls_raw = A.params + A.nets.ls_off;
            float x[NACT], s[NACT], lp = 0.0f;
#pragma unroll
            for (int c = 0; c < NACT; ++c) {
                const float ls = fminf(fmaxf(ls_raw[c], A.hp.ls_min), A.hp.ls_max);
                s[c] = expf(ls);
                x[c] = (A.act[(size_t)row * NACT + c] - y4(0)[r * P4 + c]) / s[c];
                lp = lp + (-0.5f * x[c] * x[c] - ls - 0.9189385332f);
            }
            const float lr_ = lp - A.logp[row];
            const float ratio = expf(lr_);
            const float adv = A.adv[row];
            const float lo = 1.0f - A.hp.clip, hi = 1.0f + A.hp.clip;
            const float s1c = ratio * adv, s2c = fminf(fmaxf(ratio, lo), hi) * adv;
            const bool inside = ratio >= lo && ratio <= hi;
            // torch.min passes the gradient to the smaller operand, half to each on a tie; clamp passes it inside [lo, hi]
            const float g = s1c < s2c ? adv : s1c > s2c ? (inside ? adv : 0.0f) : 0.5f * adv + (inside ? 0.5f * adv : 0.0f);
            const float dlp = -g * inv_n * ratio;
#pragma unroll
            for (int c = 0; c < NACT; ++c) {
                dz[c] = dlp * x[c] / s[c];
                t[c] = dlp * (x[c] * x[c] - 1.0f);
            }
            t[8] = (ratio - 1.0f) - lr_;
            t[9] = -fminf(s1c, s2c);
            const float v = y4(1)[r * P4], vo = A.val[row], d = v - vo;
            const float vp = vo + fminf(fmaxf(d, -A.hp.vclip), A.hp.vclip);
            const float err = A.ret[row] - vp;
            t[10] = A.hp.vscale * err * err;
            dzv = (d >= -A.hp.vclip && d <= A.hp.vclip) ? -2.0f * A.hp.vscale * err * inv_n : 0.0f;
            if (A.mean_out)
                for (int c = 0; c < NACT; ++c) A.mean_out[(size_t)(row0 + r) * NACT + c] = y4(0)[r * P4 + c];
            if (A.value_out) A.value_out[row0 + r] = v;
            float *g4p = gmat(0, S_D4) + (size_t)(row0 + r) * 8, *g4v = gmat(1, S_D4) + (size_t)(row0 + r) * 8;
#pragma unroll
            for (int c = 0; c < NACT; ++c) { g4p[c] = dz[c]; g4v[c] = c == 0 ? dzv : 0.0f; }
        }
#pragma unroll
        for (int c = 0; c < NACT; ++c) { y4(0)[r * P4 + c] = dz[c]; y4(1)[r * P4 + c] = c == 0 ? dzv : 0.0f; }
#pragma unroll
        for (int i = 0; i < PART; ++i) rowterm[r * 16 + i] = t[i];
    }
    __syncthreads();
    if (tid < PART) {
        float s = 0.0f;
        for (int r = 0; r < RB; ++r) s += rowterm[r * 16 + tid];
        A.part[(size_t)blockIdx.x * PART + tid] = s;
    }

    // ---- backward dA_l = dZ_{l+1} W_{l+1} on the MFMA (n as k, ascending quads), dZ_l = dA_l ELU'(y_l) written over y_l
    auto back = [&](int l, auto dz_of, int dzp, int Nn_fixed, auto y_of, int yp, int slot) __attribute__((always_inline)) {
        // l: the layer whose weights are multiplied (l + 1 in the text above, 0-based: 1 .. 3); output width LK[l]
        const int TK = LK[l] / 16, G = LK[l] / 16;
        for (int tt = wave; tt < 2 * TK; tt += RT / 64) {
            const int net = tt / TK, tk = tt - net * TK;
            const int Nn = Nn_fixed > 0 ? Nn_fixed : A.nets.nout[net];
            const float *dz = dz_of(net), *Wp = Wl(net, l);
            const int kcol = 16 * tk + arow;
            v4f acc = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
            for (int q = 0; q < cdiv(Nn, 4); ++q) {
                const int nn = 4 * q + akq;
                const float a = nn < Nn ? dz[arow * dzp + nn] : 0.0f;
                const float b = nn < Nn ? w_at(Wp, G, nn, kcol) : 0.0f;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
            }
            float *y = y_of(net), *g = gmat(net, slot);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = 4 * akq + j;
                const float yv = y[r * yp + kcol];
                const float d = yv > 0.0f ? acc[j] : acc[j] * (yv + 1.0f);
                y[r * yp + kcol] = d;
                if (r < rows) g[(size_t)(row0 + r) * LK[l] + kcol] = d;
            }
        }
        __syncthreads();
    };
    back(3, y4, P4, 0, y3, P3, S_D3);            // -> dZ3 (64)
    back(2, y3, P3, LN[2], y2, P2, S_D2);        // -> dZ2 (128)
    back(1, y2, P2, LN[1], y1, P1, S_D1);        // -> dZ1 (256); no input gradient for layer 1
}

// ---- dW = dZ^T A, one workgroup per (network, layer, column tile t, k tile g); g == G: the bias tile (A = 1)
struct WgradArgs {
    LiftNets nets;
    const float *ws;
    const rover_lift_ppo_state *st;
    int n;
    float *grad;
    int jobs[2][NL + 1];   // prefix sums of the per-layer job counts, per network
};
__global__ __launch_bounds__(FT) void lift_wgrad_kernel(WgradArgs A)
{
    if (stopped(A.st)) return;
    __shared__ float part[4][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int job = blockIdx.x, net = 0;
    if (job >= A.jobs[0][NL]) { job -= A.jobs[0][NL]; net = 1; }
    int l = 0;
    while (job >= A.jobs[net][l + 1]) ++l;
    job -= A.jobs[net][l];
    const int K = LK[l], N = l < NL - 1 ? LN[l] : A.nets.nout[net], G = cdiv(K, 16);
    const int t = job / (G + 1), g = job - t * (G + 1);
    const bool bias = g == G;
    const int n = A.n;
    static constexpr int dz_slot[NL] = {S_D1, S_D2, S_D3, S_D4};
    static constexpr int dz_w[NL] = {256, 128, 64, 8};
    static constexpr int a_slot[NL] = {S_X, S_Y1, S_Y2, S_Y3};
    const float *dz = A.ws + ((size_t)net * S_ROW + dz_slot[l]) * n;
    const float *am = A.ws + ((size_t)(l == 0 ? 0 : net) * S_ROW + a_slot[l]) * n;   // the standardised rows are stored once
    const int dzw = dz_w[l], aw = K;
    const int rr = lane >> 4, cc = lane & 15;
    const int col = 16 * t + cc, kin = 16 * g + cc;
    const bool col_ok = col < N, k_ok = !bias && kin < K;
    const int nq = cdiv(n, 4);
    v4f acc = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    // A operand: lane (i = cc, k = rr) = dZ[row][16 t + cc]; B operand: lane (k = rr, j = cc) = A[row][16 g + cc]
    for (int q0 = wave; q0 < nq; q0 += 16) {
        float a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = 4 * (q0 + 4 * u) + rr;
            const bool ok = r < n;
            a[u] = ok && col_ok ? dz[(size_t)r * dzw + col] : 0.0f;
            b[u] = bias ? (ok ? 1.0f : 0.0f) : (ok && k_ok ? am[(size_t)r * aw + kin] : 0.0f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u], acc, 0, 0, 0);
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) part[wave][(4 * rr + jj) * 16 + cc] = acc[jj];
    __syncthreads();
    float *gbase = A.grad + A.nets.net_off[net];
    if (!bias) {
        // packed position e = lane' * 4 + j': n = 16 t + (lane' & 15), k = 16 g + 4 j' + (lane' >> 4)
        const int lp = tid >> 2, jp = tid & 3, i = lp & 15, j = 4 * jp + (lp >> 4);
        const float s = (part[0][i * 16 + j] + part[1][i * 16 + j]) + (part[2][i * 16 + j] + part[3][i * 16 + j]);
        const bool ok = 16 * t + i < N && 16 * g + j < K;
        gbase[A.nets.w_off[net][l] + (((size_t)t * G + g) * 64 + lp) * 4 + jp] = ok ? s : 0.0f;
    } else if (tid < 16) {
        const int i = tid, c = 16 * t + i;
        const float s = (part[0][i * 16] + part[1][i * 16]) + (part[2][i * 16] + part[3][i * 16]);
        if (c < ((N + 3) & ~3)) gbase[A.nets.b_off[net][l] + c] = c < N ? s : 0.0f;
    }
}

__global__ __launch_bounds__(FT) void lift_mb_final_kernel(const float *part, int nblocks, int n, uint32_t ls_off, LiftHp hp,
                                                           const float *params, float *grad, float *stats, rover_lift_ppo_state *st)
{
    if (stopped(st)) return;
    __shared__ float red[FT];
    float tot[11];
    for (int i = 0; i < 11; ++i) {
        float s = 0.0f;
        for (int b = threadIdx.x; b < nblocks; b += FT) s += part[(size_t)b * PART + i];
        tot[i] = block_sum(s, red);
    }
    if (threadIdx.x == 0) {
        const float inv_n = 1.0f / (float)n;
        for (int i = 0; i < NACT; ++i) {
            const float ls = params[ls_off + i];
            grad[ls_off + i] = (ls >= hp.ls_min && ls <= hp.ls_max) ? tot[i] : 0.0f;   // clamp passes the gradient inside
        }
        const float kl = tot[8] * inv_n;
        stats[0] = kl;
        stats[1] = tot[9] * inv_n;
        stats[2] = tot[10] * inv_n;
        stats[3] = 0.0f;
        st->recorded += 1;
        if (hp.kl_stop > 0.0f && kl > hp.kl_stop) st->stop = 1;   // skrl: `if kl_threshold and kl_divergence > kl_threshold: break`
    }
}

// ---- clip_grad_norm_ + Adam (rover_ppo_apply's arithmetic), skipped while the epoch's stop word is set
__global__ __launch_bounds__(FT) void lift_sumsq_kernel(const float *grad, int P, float *part, const rover_lift_ppo_state *st)
{
    if (stopped(st)) return;
    __shared__ float red[FT];
    const float tot = block_sum(sumsq_partial(grad, P, NORM_BLOCKS, FT), red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
__global__ __launch_bounds__(FT) void lift_adam_prep_kernel(const float *part, float max_norm, float beta1, float beta2,
                                                            rover_lift_ppo_state *st)
{
    if (stopped(st)) return;
    __shared__ float red[FT];
    const float tot = block_sum((int)threadIdx.x < NORM_BLOCKS ? part[threadIdx.x] : 0.0f, red);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(tot);
        st->grad_norm = norm;
        st->clip_coef = grad_clip_coef(norm, max_norm);
        st->step += 1;
        adam_scalars(st->step, beta1, beta2, st->lr, &st->step_size, &st->bc2_sqrt);
    }
}
__global__ __launch_bounds__(FT) void lift_adam_kernel(float *params, float *grad, float *m, float *v, const rover_lift_ppo_state *st,
                                                       int P, float beta1, float beta2, float eps, float *rep_a, float *rep_b,
                                                       uint32_t Pa, uint32_t Pb, int n_copies)
{
    if (stopped(st)) return;
    const int e = blockIdx.x * FT + threadIdx.x;
    if (e >= P) return;
    const float p = adam_element_clipped(params, grad, m, v, e, &st->clip_coef, &st->step_size, &st->bc2_sqrt, beta1, beta2, eps);
    if ((uint32_t)e < Pa) {
        if (rep_a)
            for (int c = 0; c < n_copies; ++c) rep_a[(size_t)c * Pa + e] = p;
    } else if ((uint32_t)e < Pa + Pb) {
        if (rep_b)
            for (int c = 0; c < n_copies; ++c) rep_b[(size_t)c * Pb + (e - Pa)] = p;
    }
}

__global__ void lift_kl_kernel(const float *stats, int nmb, float thr, float factor, float lr_min, float lr_max,
                               rover_lift_ppo_state *st, float *kl_out)
{
    const int nrec = min(st->recorded, nmb);
    float s = 0.0f;
    for (int i = 0; i < nrec; ++i) s += stats[4 * i];
    if (nrec > 0) {
        const float kl = s / (float)nrec;
        st->lr = kl_adaptive_lr(st->lr, kl, thr, factor, lr_min, lr_max);
        if (kl_out) *kl_out = kl;
    } else if (kl_out) {
        *kl_out = NAN;
    }
    st->epochs += 1;
    if (st->stop) st->stopped_epochs += 1;
    st->stop = 0;
    st->recorded = 0;
}

// ---- host helpers
// rover_lift_policy_desc(nout) with the offsets rover_policy_pack sets
bool is_lift(const rover_policy_desc *d, int nout)
{
    if (!d) return false;
    if (d->obs_dim != OBS || d->prop_dim != OBS || d->n_enc != 0 || d->n_mlp != NL) return false;
    size_t off = 0;
    for (int i = 0; i < NL; ++i) {
        const rover_policy_layer &l = d->layers[i];
        if (l.K != LK[i] || l.N != (i < NL - 1 ? LN[i] : nout)) return false;
        if (l.act != (i < NL - 1 ? ROVER_ACT_ELU : ROVER_ACT_NONE) || l.split_k != 0) return false;
        if (l.w_off != off) return false;
        off += layer_weight_floats(l);
        if (l.b_off != off) return false;
        off += layer_bias_floats(l);
    }
    return true;
}
int check_pair(const rover_policy_desc *pa, const rover_policy_desc *pb)
{
    if (!pa || !pb) return rover_internal_fail(ROVER_ERR_INVALID, "descriptor is NULL");
    if (!is_lift(pa, NACT) || !is_lift(pb, 1))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "the fused lift PPO update runs the lift networks only (policy: "
                                                          "rover_lift_policy_desc(8), value: (1), packed by rover_policy_pack)");
    return ROVER_OK;
}
LiftNets nets_of(const rover_policy_desc *pa, const rover_policy_desc *pb)
{
    LiftNets s;
    const rover_policy_desc *d[2] = {pa, pb};
    s.net_floats[0] = (uint32_t)packed_floats(pa);
    s.net_floats[1] = (uint32_t)packed_floats(pb);
    s.net_off[0] = 0;
    s.net_off[1] = s.net_floats[0];
    s.ls_off = s.net_floats[0] + s.net_floats[1];
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < NL; ++i) { s.w_off[k][i] = d[k]->layers[i].w_off; s.b_off[k][i] = d[k]->layers[i].b_off; }
    s.nout[0] = NACT;
    s.nout[1] = 1;
    return s;
}
LiftHp hp_of(const rover_lift_ppo_hparams *h)
{
    return {h->clip_ratio, h->value_clip, h->value_loss_scale, h->log_std_min, h->log_std_max, h->kl_early_stop, h->scaler_eps,
            h->scaler_clip};
}
size_t ws_floats(int n) { return WS_HEAD + (size_t)2 * S_ROW * n + (size_t)PART * cdiv(n, RB); }
// statistics + merge of a scaler update (x rows gathered by idx when not NULL)
int scaler_train(double *scaler, int width, const float *x, const int64_t *idx, int rows, const rover_lift_ppo_state *st, float *ws,
                 hipStream_t s)
{
    double *bstats = reinterpret_cast<double *>(ws + WS_STATS);
    hipLaunchKernelGGL(lift_scaler_stats_kernel, dim3(width), dim3(FT), 0, s, x, idx, rows, width, st, bstats);
    if (int rc = launched("lift_scaler_stats_kernel launch: %s")) return rc;
    hipLaunchKernelGGL(lift_scaler_merge_kernel, dim3(1), dim3(MAX_SCALER_W), 0, s, scaler, width, rows, st, (const double *)bstats);
    return launched("lift_scaler_merge_kernel launch: %s");
}

}  // namespace

extern "C" {

int rover_lift_ppo_default_hparams(rover_lift_ppo_hparams *h)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "hparams is NULL");
    h->gamma = 0.99f; h->lam = 0.95f;
    h->clip_ratio = 0.2f; h->value_clip = 0.2f; h->value_loss_scale = 2.0f;
    h->log_std_min = -20.0f; h->log_std_max = 2.0f;
    h->max_grad_norm = 1.0f;
    h->beta1 = 0.9f; h->beta2 = 0.999f; h->eps = 1e-8f;
    h->kl_threshold = 0.008f; h->lr_factor = 1.5f; h->lr_min = 1e-6f; h->lr_max = 1e-2f;
    h->kl_early_stop = 0.008f;
    h->reward_scale = 0.01f;
    h->scaler_eps = 1e-8f; h->scaler_clip = 5.0f;
    return ROVER_OK;
}
size_t rover_lift_ppo_hparams_bytes(void) { return sizeof(rover_lift_ppo_hparams); }
size_t rover_lift_ppo_state_bytes(void) { return sizeof(rover_lift_ppo_state); }

size_t rover_lift_ppo_param_floats(const rover_policy_desc *policy, const rover_policy_desc *value)
{
    if (!is_lift(policy, NACT) || !is_lift(value, 1)) return 0;
    return packed_floats(policy) + packed_floats(value) + NACT;
}
size_t rover_lift_ppo_workspace_bytes(int32_t max_rows) { return max_rows > 0 ? sizeof(float) * ws_floats(max_rows) : 0; }
size_t rover_lift_ppo_scaler_doubles(int32_t width) { return width >= 1 && width <= MAX_SCALER_W ? 2 * (size_t)width + 1 : 0; }

int rover_lift_ppo_standardize(const rover_lift_ppo_hparams *h, double *scaler, int32_t width, const float *x, int32_t rows,
                               int32_t train, int32_t inverse, float *out, void *ws, size_t ws_bytes, void *stream)
{
    if (!h || !scaler || !x || !out) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (width < 1 || width > MAX_SCALER_W) return rover_internal_fail(ROVER_ERR_INVALID, "width must be in [1, 64]");
    if (rows < 1 || (train && rows < 2)) return rover_internal_fail(ROVER_ERR_INVALID, "rows must be >= 1 (>= 2 to train)");
    if (train && inverse) return rover_internal_fail(ROVER_ERR_INVALID, "train and inverse are exclusive");
    if (train && (!ws || ws_bytes < rover_lift_ppo_workspace_bytes(1)))
        return rover_internal_fail(ROVER_ERR_INVALID, "lift PPO workspace too small");
    if (reinterpret_cast<uintptr_t>(scaler) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "scaler must be 8-byte aligned");
    int dev;
    if (int rc = device_of(scaler, &dev)) return rc;
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (train)
        if (int rc = scaler_train(scaler, width, x, nullptr, rows, nullptr, static_cast<float *>(ws), s)) return rc;
    const size_t total = (size_t)rows * width;
    hipLaunchKernelGGL(lift_scaler_apply_kernel, dim3((unsigned)((total + FT - 1) / FT)), dim3(FT), 0, s, (const double *)scaler,
                       (int)width, x, (int)rows, (int)(inverse != 0), h->scaler_eps, h->scaler_clip, out);
    return launched("lift_scaler_apply_kernel launch: %s");
}

int rover_lift_ppo_minibatch(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_lift_ppo_hparams *h,
                             const float *params, double *state_scaler, const float *obs, const float *act, const float *logp,
                             const float *val, const float *ret, const float *adv, const int64_t *idx, int32_t n,
                             int32_t train_scaler, void *state, void *ws, size_t ws_bytes, float *grad, float *stats,
                             float *mean_out, float *value_out, void *stream)
{
    if (int rc = check_pair(policy, value)) return rc;
    if (!h || !params || !state_scaler || !obs || !act || !logp || !val || !ret || !adv || !idx || !state || !ws || !grad || !stats)
        return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (n < 1 || (train_scaler && n < 2)) return rover_internal_fail(ROVER_ERR_INVALID, "n must be >= 1 (>= 2 to train the scaler)");
    if (ws_bytes < rover_lift_ppo_workspace_bytes(n)) return rover_internal_fail(ROVER_ERR_INVALID, "lift PPO workspace too small");
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(params)) & 15)
        return rover_internal_fail(ROVER_ERR_INVALID, "workspace and parameters must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(state_scaler)) & 7)
        return rover_internal_fail(ROVER_ERR_INVALID, "state and scaler must be 8-byte aligned");
    int dev;
    if (int rc = device_of(params, &dev)) return rc;
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    rover_lift_ppo_state *st = static_cast<rover_lift_ppo_state *>(state);
    float *wsf = static_cast<float *>(ws);
    if (train_scaler)
        if (int rc = scaler_train(state_scaler, OBS, obs, idx, n, st, wsf, s)) return rc;
    RowsArgs R;
    R.nets = nets_of(policy, value);
    R.hp = hp_of(h);
    R.params = params; R.obs = obs; R.act = act; R.logp = logp; R.val = val; R.ret = ret; R.adv = adv; R.idx = idx; R.n = n;
    R.scaler = state_scaler; R.st = st;
    R.ws = wsf + WS_HEAD;
    R.part = R.ws + (size_t)2 * S_ROW * n;
    R.mean_out = mean_out; R.value_out = value_out;
    const int nblk = cdiv(n, RB);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(lift_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)(sizeof(float) * ROWS_LDS_FLOATS));
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(lift_rows_kernel, dim3(nblk), dim3(RT), sizeof(float) * ROWS_LDS_FLOATS, s, R);
    if (int rc = launched("lift_rows_kernel launch: %s")) return rc;
    WgradArgs W;
    W.nets = R.nets; W.ws = R.ws; W.st = st; W.n = n; W.grad = grad;
    for (int k = 0; k < 2; ++k) {
        W.jobs[k][0] = 0;
        for (int l = 0; l < NL; ++l) {
            const int N = l < NL - 1 ? LN[l] : R.nets.nout[k];
            W.jobs[k][l + 1] = W.jobs[k][l] + cdiv(N, 16) * (cdiv(LK[l], 16) + 1);
        }
    }
    hipLaunchKernelGGL(lift_wgrad_kernel, dim3(W.jobs[0][NL] + W.jobs[1][NL]), dim3(FT), 0, s, W);
    if (int rc = launched("lift_wgrad_kernel launch: %s")) return rc;
    hipLaunchKernelGGL(lift_mb_final_kernel, dim3(1), dim3(FT), 0, s, (const float *)R.part, nblk, (int)n, R.nets.ls_off, R.hp,
                       params, grad, stats, st);
    return launched("lift_mb_final_kernel launch: %s");
}

int rover_lift_ppo_apply(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_lift_ppo_hparams *h,
                         float *params, float *grad, float *adam_m, float *adam_v, void *state, float *replicas_policy,
                         float *replicas_value, int32_t n_copies, void *ws, size_t ws_bytes, void *stream)
{
    if (int rc = check_pair(policy, value)) return rc;
    if (!h || !params || !grad || !adam_m || !adam_v || !state || !ws) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if ((replicas_policy || replicas_value) && n_copies < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n_copies must be >= 1");
    if (ws_bytes < rover_lift_ppo_workspace_bytes(1)) return rover_internal_fail(ROVER_ERR_INVALID, "lift PPO workspace too small");
    if (reinterpret_cast<uintptr_t>(state) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "state must be 8-byte aligned");
    int dev;
    if (int rc = device_of(params, &dev)) return rc;
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const LiftNets nets = nets_of(policy, value);
    const int P = (int)(nets.ls_off + NACT);
    float *part = static_cast<float *>(ws);
    rover_lift_ppo_state *st = static_cast<rover_lift_ppo_state *>(state);
    hipLaunchKernelGGL(lift_sumsq_kernel, dim3(NORM_BLOCKS), dim3(FT), 0, s, (const float *)grad, P, part, (const rover_lift_ppo_state *)st);
    if (int rc = launched("lift_sumsq_kernel launch: %s")) return rc;
    hipLaunchKernelGGL(lift_adam_prep_kernel, dim3(1), dim3(FT), 0, s, (const float *)part, h->max_grad_norm, h->beta1, h->beta2, st);
    if (int rc = launched("lift_adam_prep_kernel launch: %s")) return rc;
    hipLaunchKernelGGL(lift_adam_kernel, dim3(cdiv(P, FT)), dim3(FT), 0, s, params, grad, adam_m, adam_v, (const rover_lift_ppo_state *)st,
                       P, h->beta1, h->beta2, h->eps, replicas_policy, replicas_value, nets.net_floats[0], nets.net_floats[1],
                       (int)n_copies);
    return launched("lift_adam_kernel launch: %s");
}

int rover_lift_ppo_kl_schedule(const rover_lift_ppo_hparams *h, const float *stats, int32_t n_minibatches, void *state,
                               float *kl_out, void *stream)
{
    if (!h || !stats || !state) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (n_minibatches < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n_minibatches must be >= 1");
    if (reinterpret_cast<uintptr_t>(state) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "state must be 8-byte aligned");
    int dev;
    if (int rc = device_of(stats, &dev)) return rc;
    DeviceGuard guard(dev);
    hipLaunchKernelGGL(lift_kl_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), stats, (int)n_minibatches,
                       h->kl_threshold, h->lr_factor, h->lr_min, h->lr_max, static_cast<rover_lift_ppo_state *>(state), kl_out);
    return launched("lift_kl_kernel launch: %s");
}

}  // extern "C"
