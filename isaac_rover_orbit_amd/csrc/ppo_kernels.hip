// ppo_kernels.hip -- fused PPO update of the rover's policy / value networks (gfx950 / CDNA4, wave64).
//
// Replaces the torch autograd update of examples/04_train_ppo.py for the reference architecture (get_models.py:36-62).
// See include/rover_train.h for the contract and the reduction order.  Kernels, per minibatch:
//   ppo_rows_kernel      one 256-thread workgroup per 16 gathered rows: forward of both networks with rover_policy_forward's
//                        exact chains (scalar fmaf in the same k order = the f32 MFMA's k-ordered chain), the closed-form loss
//                        gradient, and the row-parallel backward dA = dZ W down to layer 1, everything in LDS; stores the
//                        activations and every dZ for the weight gradients, plus per-workgroup partials;
//   ppo_wgrad_kernel     one workgroup per 16 x 16 tile of a weight gradient (or of a bias gradient), dW = dZ^T A on
//                        v_mfma_f32_16x16x4_f32 with the rows as k, written in the packed layout;
//   ppo_mb_final_kernel  one workgroup: log_std gradient, KL and loss terms from the partials.
// and per optimiser step ppo_sumsq_kernel -> ppo_adam_prep_kernel -> ppo_adam_kernel (norm, clip, Adam, replica refresh); their
// arithmetic, the KL rate rule, the packed-layout helpers and the reference-architecture check are train_shared.hpp's, device_of and
// launched rover_internal.hpp's.
// Each of the six has a gated twin for skrl's KL early stop (include/rover_train_gate.h): the same code behind one load of
// rover_ppo_epoch.stop -- the rows and wgrad kernels as a second instantiation over a wider argument struct, the four small ones as
// *_gated_kernel around a shared device function; ppo_epoch_end_kernel closes an epoch.
//
// The backward reads W[n][k] straight from the packed (B-fragment ordered) parameter vector by index, neither a transposed copy
// nor an LDS stage: a thread owns one input column k for 16 rows and reads each W[n][k] once per 16 rows, so the 160 KB of
// weights per workgroup pass through L1 / L2 once; a transposed copy would be one more buffer to refresh after every step.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_hip.h"
#include "../../include/rover_policy.h"
#include "../../include/rover_train.h"
#include "../../include/rover_train_gate.h"
#include "rover_internal.hpp"
#include "train_math.hpp"
#include "train_shared.hpp"

namespace {

constexpr int OBS = 965, PROP = 4, ENC_OFF = 3;
constexpr int NL = 6;
constexpr int LK[NL] = {961, 80, 64, 256, 160, 128};          // in features of the reference layers
constexpr int LN[NL - 1] = {80, 60, 256, 160, 128};          // out features of layers 1 .. 5 (layer 6: 2 policy, 1 value)
constexpr int RB = 16;                                       // rows per workgroup of ppo_rows_kernel
constexpr int FT = 256;                                      // threads of every multi-thread kernel here
constexpr int TP = 968;                                      // LDS pitch of a staged observation row (column c at 1 + c:
                                                             // the encoder's column 3 lands 16-byte aligned)
constexpr int W1 = 80, WM = 64, W3 = 256, W4 = 160, W5 = 128, WY = 4;   // LDS activation widths (WM: the MLP input 4 + 60)
constexpr int NET_F = RB * (W1 + WM + W3 + W4 + W5 + WY);
constexpr int ROWS_LDS_BYTES = 4 * (RB * TP + 2 * NET_F);
// workspace: [0, 256) apply partials; then per network the matrices below, each (n, width) row-major; then 8 floats per
// ppo_rows_kernel workgroup
constexpr int WS_HEAD = 256;
enum { S_A1 = 0, S_M = 80, S_A3 = 144, S_A4 = 400, S_A5 = 560, S_DZ1 = 688, S_DZ2 = 768, S_DZ3 = 828, S_DZ4 = 1084, S_DZ5 = 1244,
       S_DZ6 = 1372, S_ROW = 1374 };
constexpr int NORM_BLOCKS = 128;

// where the parameters of each network and log_std sit in the flat vector (offsets in floats)
struct PpoNets {
    uint32_t net_off[2];          // start of the policy / value packed block
    uint32_t w_off[2][NL], b_off[2][NL];
    uint32_t ls_off;              // log_std
    uint32_t net_floats[2];       // packed floats per network (one replica)
    int32_t nout[2];              // 2, 1
    float slope;
};
struct PpoHp {
    float clip, vclip, vscale, ls_min, ls_max;
};

// acc[r] = chain_k fmaf(in[r][k], W[n][k], acc[r]) for k in [k0, k1) ascending, r < 16 (the MFMA's k-ordered chain)
__device__ __forceinline__ void chain16(float (&acc)[RB], const float *in, int ip, const float *Wp, int G, int n, int k0, int k1)
{
    int k = k0;
#pragma unroll 1   // K is a constant after inlining: a full unroll hoists every group's LDS reads and spills
    for (; k + 16 <= k1; k += 16) {   // whole k groups (k0 is a multiple of 16): four float4 fragments = W[n][16 g .. 16 g + 15]
        asm volatile("" ::: "memory");   // the rows are the same for every column: keep LICM from hoisting them (spills)
        const v4f *f = reinterpret_cast<const v4f *>(Wp) + (((size_t)(n >> 4) * G + (k >> 4)) * 64 + (n & 15));
        const v4f q0 = f[0], q1 = f[16], q2 = f[32], q3 = f[48];   // q_m[j] = W[n][16 g + 4 j + m]
        const float w[16] = {q0[0], q1[0], q2[0], q3[0], q0[1], q1[1], q2[1], q3[1],
                             q0[2], q1[2], q2[2], q3[2], q0[3], q1[3], q2[3], q3[3]};
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const v4f *x = reinterpret_cast<const v4f *>(in + r * ip + k);
            const v4f x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
            float a = acc[r];
            a = fmaf(x0[0], w[0], a); a = fmaf(x0[1], w[1], a); a = fmaf(x0[2], w[2], a); a = fmaf(x0[3], w[3], a);
            a = fmaf(x1[0], w[4], a); a = fmaf(x1[1], w[5], a); a = fmaf(x1[2], w[6], a); a = fmaf(x1[3], w[7], a);
            a = fmaf(x2[0], w[8], a); a = fmaf(x2[1], w[9], a); a = fmaf(x2[2], w[10], a); a = fmaf(x2[3], w[11], a);
            a = fmaf(x3[0], w[12], a); a = fmaf(x3[1], w[13], a); a = fmaf(x3[2], w[14], a); a = fmaf(x3[3], w[15], a);
            acc[r] = a;
        }
    }
#pragma unroll 1
    for (; k < k1; ++k) {            // the ragged end of the 961-wide layer
        asm volatile("" ::: "memory");
        const float w = w_at(Wp, G, n, k);
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = fmaf(in[r * ip + k], w, acc[r]);
    }
}
// the split-K pre-activation: 8 contiguous ranges of ceil(G / 8) * 16 inputs, ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))
__device__ __forceinline__ void split_chain16(float (&out)[RB], const float *in, int ip, const float *Wp, int K, int n)
{
    const int G = cdiv(K, 16), R = 16 * cdiv(G, 8);
    float s[RB], u[RB], p[RB];
#pragma unroll 1   // a real loop: straight-line ranges let the compiler hoist every range's LDS reads (spills)
    for (int i = 0; i < 8; ++i) {
        float c[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) c[r] = 0.0f;
        chain16(c, in, ip, Wp, G, n, min(i * R, K), min((i + 1) * R, K));
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            if ((i & 1) == 0) { p[r] = c[r]; continue; }
            const float pair = p[r] + c[r];
            if (i == 1) s[r] = pair;
            else if (i == 3) s[r] = s[r] + pair;
            else if (i == 5) u[r] = pair;
            else out[r] = s[r] + (u[r] + pair);
        }
    }
}

struct RowsArgs {
    PpoNets nets;
    PpoHp hp;
    const float *params, *obs, *act, *logp, *val, *ret, *adv;
    const int64_t *idx;
    int n;
    float *ws;          // the matrices (past WS_HEAD)
    float *part;        // 8 floats per workgroup
    float *mean_out, *value_out;
    static constexpr bool gated = false;
};
// The gated twins (include/rover_train_gate.h) take the same arguments and the stop word: the same kernel text behind one load and
// a branch the whole grid takes the same way.  Nothing with more than one workgroup writes the word.  The two big kernels are
// templates over their argument struct, so the ungated instantiation is the kernel it always was, instruction for instruction.
struct RowsArgsGated : RowsArgs {
    const int32_t *stop;
    static constexpr bool gated = true;
};

template <class ARGS>
__global__ __launch_bounds__(FT) void ppo_rows_kernel(ARGS A)
{
    if constexpr (ARGS::gated) {
        if (*A.stop) return;
    }
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * RB, rows = min(RB, A.n - row0), n = A.n;
    const float slope = A.nets.slope;
    float *tile = lds + 1;                                   // row r, column c at tile[r * TP + c]
    auto nbuf = [&](int net) __attribute__((always_inline)) { return lds + RB * TP + net * NET_F; };
    auto a1 = [&](int net) __attribute__((always_inline)) { return nbuf(net); };
    auto mb = [&](int net) __attribute__((always_inline)) { return nbuf(net) + RB * W1; };
    auto a3 = [&](int net) __attribute__((always_inline)) { return mb(net) + RB * WM; };
    auto a4 = [&](int net) __attribute__((always_inline)) { return a3(net) + RB * W3; };
    auto a5 = [&](int net) __attribute__((always_inline)) { return a4(net) + RB * W4; };
    auto yb = [&](int net) __attribute__((always_inline)) { return a5(net) + RB * W5; };
    auto gmat = [&](int net, int slot) __attribute__((always_inline)) { return A.ws + ((size_t)net * S_ROW + slot) * n; };
    auto Wl = [&](int net, int l) __attribute__((always_inline)) { return A.params + A.nets.net_off[net] + A.nets.w_off[net][l]; };
    auto Bl = [&](int net, int l) __attribute__((always_inline)) { return A.params + A.nets.net_off[net] + A.nets.b_off[net][l]; };

    // ---- gather the rows (64-bit row offsets), zero rows past n
    for (int e = tid; e < RB * OBS; e += FT) {
        const int r = e / OBS, c = e - r * OBS;
        tile[r * TP + c] = r < rows ? A.obs[(size_t)A.idx[row0 + r] * OBS + c] : 0.0f;
    }
    __syncthreads();

    // ---- forward, both networks; every thread owns (network, output column) items and 16 rows
    auto store = [&](float *dst, int pitch, int col, const float (&v)[RB], float *g, int gw) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            dst[r * pitch + col] = v[r];
            if (r < rows) g[(size_t)(row0 + r) * gw + col] = v[r];
        }
    };
    for (int it = tid; it < 2 * W1; it += FT) {             // layer 1: 961 -> 80, split-K
        const int net = it / W1, c = it - net * W1;
        float acc[RB];
        split_chain16(acc, tile + ENC_OFF, TP, Wl(net, 0), LK[0], c);
        const float b = Bl(net, 0)[c];
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = leaky(acc[r] + b, slope);
        store(a1(net), W1, c, acc, gmat(net, S_A1), W1);
    }
    for (int e = tid; e < 2 * RB * PROP; e += FT) {         // cat([states[:, :4], encoder]) (models.py:93-96)
        const int net = e / (RB * PROP), r = (e / PROP) % RB, c = e % PROP;
        mb(net)[r * WM + c] = tile[r * TP + c];
        if (r < rows) gmat(net, S_M)[(size_t)(row0 + r) * WM + c] = tile[r * TP + c];
    }
    __syncthreads();
    auto full_layer = [&](int l, int N, auto in_of, int ip, auto out_of, int op, int col0, int slot) __attribute__((always_inline)) {
        for (int it = tid; it < 2 * N; it += FT) {
            const int net = it / N, c = it - net * N;
            float acc[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) acc[r] = 0.0f;
            chain16(acc, in_of(net), ip, Wl(net, l), LK[l] / 16, c, 0, LK[l]);
            const float b = Bl(net, l)[c];
#pragma unroll
            for (int r = 0; r < RB; ++r) acc[r] = leaky(acc[r] + b, slope);
            store(out_of(net), op, col0 + c, acc, gmat(net, slot), op);
        }
        __syncthreads();
    };
    full_layer(1, LN[1], a1, W1, mb, WM, PROP, S_M);      // 80 -> 60 behind the proprioceptive columns
    full_layer(2, LN[2], mb, WM, a3, W3, 0, S_A3);         // 64 -> 256
    full_layer(3, LN[3], a3, W3, a4, W4, 0, S_A4);         // 256 -> 160
    full_layer(4, LN[4], a4, W4, a5, W5, 0, S_A5);         // 160 -> 128
    if (tid < A.nets.nout[0] + A.nets.nout[1]) {            // layer 6: 128 -> {2 + tanh, 1}, split-K
        const int net = tid >= A.nets.nout[0], c = tid - net * A.nets.nout[0];
        float acc[RB];
        split_chain16(acc, a5(net), W5, Wl(net, 5), LK[5], c);
        const float b = Bl(net, 5)[c];
#pragma unroll
        for (int r = 0; r < RB; ++r) yb(net)[r * WY + c] = net ? acc[r] + b : rv_tanhf(acc[r] + b);
    }
    __syncthreads();

    // ---- the loss and dL/d(out) per row (examples/04_train_ppo.py), sums of the row terms for this workgroup
    float *rowterm = lds;          // the tile is dead: [16][8] row terms (dls0, dls1, kl, policy loss, value loss)
    if (tid < RB) {
        const int r = tid;
        float t[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        float dz0 = 0.0f, dz1 = 0.0f, dzv = 0.0f;
        if (r < rows) {
            const int64_t row = A.idx[row0 + r];
            const float inv_n = 1.0f / (float)n;
            const float *ls_raw = A.params + A.nets.ls_off;
            const float m0 = yb(0)[r * WY], m1 = yb(0)[r * WY + 1], v = yb(1)[r * WY];
            const float ls0 = fminf(fmaxf(ls_raw[0], A.hp.ls_min), A.hp.ls_max), ls1 = fminf(fmaxf(ls_raw[1], A.hp.ls_min), A.hp.ls_max);
            const float s0 = expf(ls0), s1 = expf(ls1);
            const float x0 = (A.act[2 * row] - m0) / s0, x1 = (A.act[2 * row + 1] - m1) / s1;
            const float lp = (-0.5f * x0 * x0 - ls0 - 0.9189385332f) + (-0.5f * x1 * x1 - ls1 - 0.9189385332f);
            const float lr_ = lp - A.logp[row];
            const float ratio = expf(lr_);
            const float adv = A.adv[row];
            const float lo = 1.0f - A.hp.clip, hi = 1.0f + A.hp.clip;
            const float s1c = ratio * adv, s2c = fminf(fmaxf(ratio, lo), hi) * adv;
            const bool inside = ratio >= lo && ratio <= hi;
            // torch.min passes the gradient to the smaller operand, half to each on a tie; clamp passes it inside [lo, hi]
            float g = s1c < s2c ? adv : s1c > s2c ? (inside ? adv : 0.0f) : 0.5f * adv + (inside ? 0.5f * adv : 0.0f);
            const float dlp = -g * inv_n * ratio;
            const float dm0 = dlp * x0 / s0, dm1 = dlp * x1 / s1;
            dz0 = dm0 * (1.0f - m0 * m0);
            dz1 = dm1 * (1.0f - m1 * m1);
            t[0] = dlp * (x0 * x0 - 1.0f);
            t[1] = dlp * (x1 * x1 - 1.0f);
            t[2] = (ratio - 1.0f) - lr_;
            t[3] = -fminf(s1c, s2c);
            const float vo = A.val[row], d = v - vo;
            const float vp = vo + fminf(fmaxf(d, -A.hp.vclip), A.hp.vclip);
            const float err = A.ret[row] - vp;
            t[4] = A.hp.vscale * err * err;
            dzv = (d >= -A.hp.vclip && d <= A.hp.vclip) ? -2.0f * A.hp.vscale * err * inv_n : 0.0f;
            if (A.mean_out) { A.mean_out[2 * (size_t)(row0 + r)] = m0; A.mean_out[2 * (size_t)(row0 + r) + 1] = m1; }
            if (A.value_out) A.value_out[row0 + r] = v;
            float *g6p = gmat(0, S_DZ6) + (size_t)(row0 + r) * 2, *g6v = gmat(1, S_DZ6) + (size_t)(row0 + r) * 2;
            g6p[0] = dz0; g6p[1] = dz1; g6v[0] = dzv; g6v[1] = 0.0f;
        }
        yb(0)[r * WY] = dz0; yb(0)[r * WY + 1] = dz1; yb(1)[r * WY] = dzv;
#pragma unroll
        for (int i = 0; i < 5; ++i) rowterm[r * 8 + i] = t[i];
    }
    __syncthreads();
    if (tid < 5) {
        float s = 0.0f;
        for (int r = 0; r < RB; ++r) s += rowterm[r * 8 + tid];
        A.part[(size_t)blockIdx.x * 8 + tid] = s;
    }

    // ---- backward dA_{l-1} = dZ_l W_l, dZ_{l-1} = dA_{l-1} LeakyReLU'(a_{l-1}) written over a_{l-1} (one thread per column)
    auto back_layer = [&](int l, int N, auto dz_of, int dzp, auto a_of, int ap, int k0, int k1, int dcol, int slot, int gw) __attribute__((always_inline)) {
        const int nk = k1 - k0;
        for (int it = tid; it < 2 * nk; it += FT) {
            const int net = it / nk, k = k0 + it - net * nk;
            const int Nn = N > 0 ? N : A.nets.nout[net];
            const float *dz = dz_of(net), *Wp = Wl(net, l);
            const int G = cdiv(LK[l], 16);
            float acc[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) acc[r] = 0.0f;
            for (int c = 0; c < Nn; ++c) {
                asm volatile("" ::: "memory");   // as in chain16: dZ is the same for every column k
                const float w = w_at(Wp, G, c, k);
#pragma unroll
                for (int r = 0; r < RB; ++r) acc[r] = fmaf(dz[r * dzp + c], w, acc[r]);
            }
            float *a = a_of(net), *g = gmat(net, slot);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const float d = a[r * ap + k] > 0.0f ? acc[r] : acc[r] * slope;
                a[r * ap + k] = d;
                if (r < rows) g[(size_t)(row0 + r) * gw + k - dcol] = d;
            }
        }
        __syncthreads();
    };
    auto mb_enc = [&](int net) __attribute__((always_inline)) { return mb(net) + PROP; };
    back_layer(5, 0, yb, WY, a5, W5, 0, W5, 0, S_DZ5, W5);          // -> dZ5 (128)
    back_layer(4, LN[4], a5, W5, a4, W4, 0, W4, 0, S_DZ4, W4);      // -> dZ4 (160)
    back_layer(3, LN[3], a4, W4, a3, W3, 0, W3, 0, S_DZ3, W3);      // -> dZ3 (256)
    back_layer(2, LN[2], a3, W3, mb, WM, PROP, WM, PROP, S_DZ2, 60);  // -> dZ2 (the encoder's 60 of the MLP input)
    back_layer(1, LN[1], mb_enc, WM, a1, W1, 0, W1, 0, S_DZ1, W1);  // -> dZ1 (80); no input gradient for layer 1
}

// ---- dW = dZ^T A, one workgroup per (network, layer, column tile t, k tile g); g == G: the bias tile (A = 1)
struct WgradArgs {
    PpoNets nets;
    const float *obs;
    const int64_t *idx;
    const float *ws;
    int n;
    float *grad;
    int jobs[2][NL + 1];   // prefix sums of the per-layer job counts, per network
    static constexpr bool gated = false;
};
struct WgradArgsGated : WgradArgs {
    const int32_t *stop;
    static constexpr bool gated = true;
};
template <class ARGS>
__global__ __launch_bounds__(FT) void ppo_wgrad_kernel(ARGS A)
{
    if constexpr (ARGS::gated) {
        if (*A.stop) return;
    }
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
    static constexpr int dz_slot[NL] = {S_DZ1, S_DZ2, S_DZ3, S_DZ4, S_DZ5, S_DZ6};
    static constexpr int dz_w[NL] = {80, 60, 256, 160, 128, 2};
    static constexpr int a_slot[NL] = {-1, S_A1, S_M, S_A3, S_A4, S_A5};
    const float *dz = A.ws + ((size_t)net * S_ROW + dz_slot[l]) * n;
    const float *am = l > 0 ? A.ws + ((size_t)net * S_ROW + a_slot[l]) * n : nullptr;
    const int dzw = dz_w[l], aw = l > 0 ? LK[l] : 0;
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
            if (bias) b[u] = ok ? 1.0f : 0.0f;
            else if (l == 0) b[u] = ok && k_ok ? A.obs[(size_t)A.idx[r] * OBS + ENC_OFF + kin] : 0.0f;
            else b[u] = ok && k_ok ? am[(size_t)r * aw + kin] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u], acc, 0, 0, 0);
    }
    // D[i][j] = dW[16 t + i][16 g + j]: lane holds i = 4 rr + jj, j = cc
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

// fixed halving tree over the 256 threads of the block; returns the total in thread 0
__device__ __forceinline__ float block_sum(float v, float *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = FT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ void ppo_mb_final_body(const float *part, int nblocks, int n, uint32_t ls_off, const PpoHp &hp,
                                                  const float *params, float *grad, float *stats)
{
    __shared__ float red[FT];
    float tot[5];
    for (int i = 0; i < 5; ++i) {
        float s = 0.0f;
        for (int b = threadIdx.x; b < nblocks; b += FT) s += part[(size_t)b * 8 + i];
        tot[i] = block_sum(s, red);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float inv_n = 1.0f / (float)n;
        for (int i = 0; i < 2; ++i) {
            const float ls = params[ls_off + i];
            grad[ls_off + i] = (ls >= hp.ls_min && ls <= hp.ls_max) ? tot[i] : 0.0f;   // clamp passes the gradient inside
        }
        grad[ls_off + 2] = 0.0f;
        grad[ls_off + 3] = 0.0f;
        stats[0] = tot[2] * inv_n;
        stats[1] = tot[3] * inv_n;
        stats[2] = tot[4] * inv_n;
        stats[3] = 0.0f;
    }
}
__global__ __launch_bounds__(FT) void ppo_mb_final_kernel(const float *part, int nblocks, int n, uint32_t ls_off, PpoHp hp,
                                                          const float *params, float *grad, float *stats)
{
    ppo_mb_final_body(part, nblocks, n, ls_off, hp, params, grad, stats);
}
// One workgroup: every thread reads the stop word on entry; thread 0 records the KL it has just written and may set the word,
// behind the barriers of the sums, so the write follows every read of this launch.
__global__ __launch_bounds__(FT) void ppo_mb_final_gated_kernel(const float *part, int nblocks, int n, uint32_t ls_off, PpoHp hp,
                                                                const float *params, float *grad, float *stats, float kl_stop,
                                                                rover_ppo_epoch *ep)
{
    if (ep->stop) return;
    ppo_mb_final_body(part, nblocks, n, ls_off, hp, params, grad, stats);
    if (threadIdx.x == 0) {
        const float kl = stats[0];
        const int32_t rec = ep->recorded;
        ep->recorded = rec + 1;
        if (kl_stop > 0.0f && kl > kl_stop) {     // strict, fp32: false for a NaN KL
            ep->stop = 1;
            ep->stop_minibatch = rec;
            ep->stop_kl = kl;
        }
    }
}

// ---- clip_grad_norm_ + Adam
__device__ __forceinline__ void ppo_sumsq_body(const float *grad, int P, float *part)
{
    __shared__ float red[FT];
    const float tot = block_sum(sumsq_partial(grad, P, NORM_BLOCKS, FT), red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
__global__ __launch_bounds__(FT) void ppo_sumsq_kernel(const float *grad, int P, float *part) { ppo_sumsq_body(grad, P, part); }
__global__ __launch_bounds__(FT) void ppo_sumsq_gated_kernel(const float *grad, int P, float *part, const int32_t *stop)
{
    if (*stop) return;
    ppo_sumsq_body(grad, P, part);
}
__device__ __forceinline__ void ppo_adam_prep_body(const float *part, float max_norm, float beta1, float beta2, rover_ppo_state *st)
{
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
__global__ __launch_bounds__(FT) void ppo_adam_prep_kernel(const float *part, float max_norm, float beta1, float beta2,
                                                           rover_ppo_state *st)
{
    ppo_adam_prep_body(part, max_norm, beta1, beta2, st);
}
__global__ __launch_bounds__(FT) void ppo_adam_prep_gated_kernel(const float *part, float max_norm, float beta1, float beta2,
                                                                 rover_ppo_state *st, const int32_t *stop)
{
    if (*stop) return;
    ppo_adam_prep_body(part, max_norm, beta1, beta2, st);
}
__device__ __forceinline__ void ppo_adam_body(float *params, float *grad, float *m, float *v, const rover_ppo_state *st, int P,
                                              float beta1, float beta2, float eps, float *rep_a, float *rep_b, uint32_t Pa,
                                              uint32_t Pb, int n_copies)
{
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
__global__ __launch_bounds__(FT) void ppo_adam_kernel(float *params, float *grad, float *m, float *v, const rover_ppo_state *st,
                                                      int P, float beta1, float beta2, float eps, float *rep_a, float *rep_b,
                                                      uint32_t Pa, uint32_t Pb, int n_copies)
{
    ppo_adam_body(params, grad, m, v, st, P, beta1, beta2, eps, rep_a, rep_b, Pa, Pb, n_copies);
}
__global__ __launch_bounds__(FT) void ppo_adam_gated_kernel(float *params, float *grad, float *m, float *v, const rover_ppo_state *st,
                                                            int P, float beta1, float beta2, float eps, float *rep_a, float *rep_b,
                                                            uint32_t Pa, uint32_t Pb, int n_copies, const int32_t *stop)
{
    if (*stop) return;
    ppo_adam_body(params, grad, m, v, st, P, beta1, beta2, eps, rep_a, rep_b, Pa, Pb, n_copies);
}

__global__ void ppo_kl_kernel(const float *stats, int nmb, float thr, float factor, float lr_min, float lr_max,
                              rover_ppo_state *st, float *kl_out)
{
    float s = 0.0f;
    for (int i = 0; i < nmb; ++i) s += stats[4 * i];
    const float kl = s / (float)nmb;
    double lr = st->lr;   // kl_adaptive_lr written out: behind the call this kernel's last branch comes out inverted
    if ((double)kl > 2.0 * (double)thr) lr = fmax(lr / (double)factor, (double)lr_min);
    else if ((double)kl < 0.5 * (double)thr) lr = fmin(lr * (double)factor, (double)lr_max);
    st->lr = lr;
    if (kl_out) *kl_out = kl;
}

// one thread: the mean of the recorded KLs, the scheduler when it is switched on, and the epoch's bookkeeping
__global__ void ppo_epoch_end_kernel(const float *stats, int nmb, float thr, float factor, float lr_min, float lr_max,
                                     rover_ppo_state *st, rover_ppo_epoch *ep, int schedule, float *kl_out)
{
    const int rec = min(max(ep->recorded, 0), nmb);
    float kl = 0.0f;
    if (rec > 0) {
        float s = 0.0f;
        for (int i = 0; i < rec; ++i) s += stats[4 * i];
        kl = s / (float)rec;
        if (schedule) st->lr = kl_adaptive_lr(st->lr, kl, thr, factor, lr_min, lr_max);
    }
    if (kl_out) *kl_out = kl;
    const int32_t stopped = ep->stopped_epochs + (ep->stop != 0);
    ep->epochs += 1;
    ep->stopped_epochs = stopped;
    if (stopped == 0) {
        ep->stop_minibatch = -1;
        ep->stop_kl = 0.0f;
    }
    ep->stop = 0;
    ep->recorded = 0;
}

__global__ __launch_bounds__(FT) void ppo_gae_kernel(const float *rew, const float *done, const float *val, const float *last_v, int T,
                                                     int n, float gamma, float gl, float *adv, float *ret)
{
    const int e = blockIdx.x * FT + threadIdx.x;
    if (e >= n) return;
    float gae = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
        const size_t i = (size_t)t * n + e;
        const float nv = t == T - 1 ? last_v[e] : val[i + n];
        const float nd = 1.0f - done[i];
        const float delta = (rew[i] + (gamma * nv) * nd) - val[i];
        gae = delta + (gl * nd) * gae;
        adv[i] = gae;
        ret[i] = gae + val[i];
    }
}

// ---- host helpers
int check_pair(const rover_policy_desc *pa, const rover_policy_desc *pb)
{
    if (!pa || !pb) return rover_internal_fail(ROVER_ERR_INVALID, "descriptor is NULL");
    if (!is_reference(pa, 2, ROVER_ACT_TANH) || !is_reference(pb, 1, ROVER_ACT_NONE))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "the fused PPO update runs the reference architecture only (policy: "
                                                          "rover_policy_default_desc(2, 1), value: (1, 0), packed by rover_policy_pack)");
    return ROVER_OK;
}
PpoNets nets_of(const rover_policy_desc *pa, const rover_policy_desc *pb)
{
    PpoNets s;
    const rover_policy_desc *d[2] = {pa, pb};
    s.net_floats[0] = (uint32_t)packed_floats(pa);
    s.net_floats[1] = (uint32_t)packed_floats(pb);
    s.net_off[0] = 0;
    s.net_off[1] = s.net_floats[0];
    s.ls_off = s.net_floats[0] + s.net_floats[1];
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < NL; ++i) { s.w_off[k][i] = d[k]->layers[i].w_off; s.b_off[k][i] = d[k]->layers[i].b_off; }
    s.nout[0] = 2;
    s.nout[1] = 1;
    s.slope = pa->leaky_slope;
    return s;
}
size_t ws_floats(int n) { return WS_HEAD + (size_t)2 * S_ROW * n + (size_t)8 * cdiv(n, RB); }

}  // namespace

extern "C" {

int rover_ppo_default_hparams(rover_ppo_hparams *h)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "hparams is NULL");
    h->gamma = 0.99f; h->lam = 0.95f;
    h->clip_ratio = 0.2f; h->value_clip = 0.2f; h->value_loss_scale = 1.0f;
    h->log_std_min = -20.0f; h->log_std_max = 2.0f;
    h->max_grad_norm = 0.5f;
    h->beta1 = 0.9f; h->beta2 = 0.999f; h->eps = 1e-8f;
    h->kl_threshold = 0.008f; h->lr_factor = 1.5f; h->lr_min = 1e-6f; h->lr_max = 1e-2f;
    return ROVER_OK;
}
size_t rover_ppo_hparams_bytes(void) { return sizeof(rover_ppo_hparams); }
size_t rover_ppo_state_bytes(void) { return sizeof(rover_ppo_state); }

size_t rover_ppo_param_floats(const rover_policy_desc *policy, const rover_policy_desc *value)
{
    if (!is_reference(policy, 2, ROVER_ACT_TANH) || !is_reference(value, 1, ROVER_ACT_NONE)) return 0;
    return packed_floats(policy) + packed_floats(value) + 4;
}
size_t rover_ppo_workspace_bytes(int32_t max_rows) { return max_rows > 0 ? sizeof(float) * ws_floats(max_rows) : 0; }

}  // extern "C"

namespace {

// rover_ppo_minibatch (ep == NULL: the ungated kernels, the launches as they always were) and rover_ppo_minibatch_gated
int minibatch_impl(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_ppo_hparams *h, const float *params,
                   const float *obs, const float *act, const float *logp, const float *val, const float *ret, const float *adv,
                   const int64_t *idx, int32_t n, void *ws, size_t ws_bytes, float *grad, float *stats, float *mean_out,
                   float *value_out, float kl_stop, rover_ppo_epoch *ep, void *stream)
{
    if (int rc = check_pair(policy, value)) return rc;
    if (!h || !params || !obs || !act || !logp || !val || !ret || !adv || !idx || !ws || !grad || !stats)
        return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (n < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n must be >= 1");
    if (ws_bytes < rover_ppo_workspace_bytes(n)) return rover_internal_fail(ROVER_ERR_INVALID, "PPO workspace too small");
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(params)) & 15)
        return rover_internal_fail(ROVER_ERR_INVALID, "workspace and parameters must be 16-byte aligned");
    int dev;
    if (int rc = device_of(params, &dev)) return rc;
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    RowsArgsGated R;
    R.stop = ep ? &ep->stop : nullptr;
    R.nets = nets_of(policy, value);
    R.hp = {h->clip_ratio, h->value_clip, h->value_loss_scale, h->log_std_min, h->log_std_max};
    R.params = params; R.obs = obs; R.act = act; R.logp = logp; R.val = val; R.ret = ret; R.adv = adv; R.idx = idx; R.n = n;
    R.ws = static_cast<float *>(ws) + WS_HEAD;
    R.part = R.ws + (size_t)2 * S_ROW * n;
    R.mean_out = mean_out; R.value_out = value_out;
    const int nblk = cdiv(n, RB);
    hipError_t e = hipFuncSetAttribute(ep ? reinterpret_cast<const void *>(ppo_rows_kernel<RowsArgsGated>)
                                          : reinterpret_cast<const void *>(ppo_rows_kernel<RowsArgs>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, ROWS_LDS_BYTES);
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    if (ep) hipLaunchKernelGGL(ppo_rows_kernel<RowsArgsGated>, dim3(nblk), dim3(FT), ROWS_LDS_BYTES, s, R);
    else hipLaunchKernelGGL(ppo_rows_kernel<RowsArgs>, dim3(nblk), dim3(FT), ROWS_LDS_BYTES, s, static_cast<const RowsArgs &>(R));
    if (int rc = launched("ppo_rows_kernel launch: %s")) return rc;
    WgradArgsGated W;
    W.stop = R.stop;
    W.nets = R.nets; W.obs = obs; W.idx = idx; W.ws = R.ws; W.n = n; W.grad = grad;
    for (int k = 0; k < 2; ++k) {
        W.jobs[k][0] = 0;
        for (int l = 0; l < NL; ++l) {
            const int N = l < NL - 1 ? LN[l] : R.nets.nout[k];
            W.jobs[k][l + 1] = W.jobs[k][l] + cdiv(N, 16) * (cdiv(LK[l], 16) + 1);
        }
    }
    if (ep) hipLaunchKernelGGL(ppo_wgrad_kernel<WgradArgsGated>, dim3(W.jobs[0][NL] + W.jobs[1][NL]), dim3(FT), 0, s, W);
    else hipLaunchKernelGGL(ppo_wgrad_kernel<WgradArgs>, dim3(W.jobs[0][NL] + W.jobs[1][NL]), dim3(FT), 0, s, static_cast<const WgradArgs &>(W));
    if (int rc = launched("ppo_wgrad_kernel launch: %s")) return rc;
    if (ep)
        hipLaunchKernelGGL(ppo_mb_final_gated_kernel, dim3(1), dim3(FT), 0, s, (const float *)R.part, nblk, (int)n, R.nets.ls_off, R.hp,
                           params, grad, stats, kl_stop, ep);
    else
        hipLaunchKernelGGL(ppo_mb_final_kernel, dim3(1), dim3(FT), 0, s, (const float *)R.part, nblk, (int)n, R.nets.ls_off, R.hp,
                           params, grad, stats);
    return launched("ppo_mb_final_kernel launch: %s");
}

// rover_ppo_apply (ep == NULL) and rover_ppo_apply_gated
int apply_impl(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_ppo_hparams *h, float *params, float *grad,
               float *adam_m, float *adam_v, void *state, float *replicas_policy, float *replicas_value, int32_t n_copies, void *ws,
               size_t ws_bytes, const rover_ppo_epoch *ep, void *stream)
{
    if (int rc = check_pair(policy, value)) return rc;
    if (!h || !params || !grad || !adam_m || !adam_v || !state || !ws) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if ((replicas_policy || replicas_value) && n_copies < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n_copies must be >= 1");
    if (ws_bytes < rover_ppo_workspace_bytes(1)) return rover_internal_fail(ROVER_ERR_INVALID, "PPO workspace too small");
    if (reinterpret_cast<uintptr_t>(state) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "state must be 8-byte aligned");
    int dev;
    if (int rc = device_of(params, &dev)) return rc;
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PpoNets nets = nets_of(policy, value);
    const int P = (int)(nets.ls_off + 4);
    float *part = static_cast<float *>(ws);
    rover_ppo_state *st = static_cast<rover_ppo_state *>(state);
    const int32_t *stop = ep ? &ep->stop : nullptr;
    if (ep) hipLaunchKernelGGL(ppo_sumsq_gated_kernel, dim3(NORM_BLOCKS), dim3(FT), 0, s, (const float *)grad, P, part, stop);
    else hipLaunchKernelGGL(ppo_sumsq_kernel, dim3(NORM_BLOCKS), dim3(FT), 0, s, (const float *)grad, P, part);
    if (int rc = launched("ppo_sumsq_kernel launch: %s")) return rc;
    if (ep)
        hipLaunchKernelGGL(ppo_adam_prep_gated_kernel, dim3(1), dim3(FT), 0, s, (const float *)part, h->max_grad_norm, h->beta1, h->beta2,
                           st, stop);
    else
        hipLaunchKernelGGL(ppo_adam_prep_kernel, dim3(1), dim3(FT), 0, s, (const float *)part, h->max_grad_norm, h->beta1, h->beta2, st);
    if (int rc = launched("ppo_adam_prep_kernel launch: %s")) return rc;
    if (ep)
        hipLaunchKernelGGL(ppo_adam_gated_kernel, dim3(cdiv(P, FT)), dim3(FT), 0, s, params, grad, adam_m, adam_v,
                           (const rover_ppo_state *)st, P, h->beta1, h->beta2, h->eps, replicas_policy, replicas_value,
                           nets.net_floats[0], nets.net_floats[1], (int)n_copies, stop);
    else
        hipLaunchKernelGGL(ppo_adam_kernel, dim3(cdiv(P, FT)), dim3(FT), 0, s, params, grad, adam_m, adam_v, (const rover_ppo_state *)st,
                           P, h->beta1, h->beta2, h->eps, replicas_policy, replicas_value, nets.net_floats[0], nets.net_floats[1],
                           (int)n_copies);
    return launched("ppo_adam_kernel launch: %s");
}

}  // namespace

extern "C" {

int rover_ppo_minibatch(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_ppo_hparams *h,
                        const float *params, const float *obs, const float *act, const float *logp, const float *val,
                        const float *ret, const float *adv, const int64_t *idx, int32_t n, void *ws, size_t ws_bytes,
                        float *grad, float *stats, float *mean_out, float *value_out, void *stream)
{
    return minibatch_impl(policy, value, h, params, obs, act, logp, val, ret, adv, idx, n, ws, ws_bytes, grad, stats, mean_out,
                          value_out, 0.0f, nullptr, stream);
}

int rover_ppo_apply(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_ppo_hparams *h, float *params,
                    float *grad, float *adam_m, float *adam_v, void *state, float *replicas_policy, float *replicas_value,
                    int32_t n_copies, void *ws, size_t ws_bytes, void *stream)
{
    return apply_impl(policy, value, h, params, grad, adam_m, adam_v, state, replicas_policy, replicas_value, n_copies, ws, ws_bytes,
                      nullptr, stream);
}

size_t rover_ppo_epoch_bytes(void) { return sizeof(rover_ppo_epoch); }

int rover_ppo_minibatch_gated(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_ppo_hparams *h,
                              const float *params, const float *obs, const float *act, const float *logp, const float *val,
                              const float *ret, const float *adv, const int64_t *idx, int32_t n, void *ws, size_t ws_bytes,
                              float *grad, float *stats, float *mean_out, float *value_out, float kl_early_stop, void *epoch,
                              void *stream)
{
    if (!epoch) return rover_internal_fail(ROVER_ERR_INVALID, "rover_ppo_minibatch_gated: epoch is NULL");
    if (reinterpret_cast<uintptr_t>(epoch) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "epoch must be 8-byte aligned");
    return minibatch_impl(policy, value, h, params, obs, act, logp, val, ret, adv, idx, n, ws, ws_bytes, grad, stats, mean_out,
                          value_out, kl_early_stop, static_cast<rover_ppo_epoch *>(epoch), stream);
}

int rover_ppo_apply_gated(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_ppo_hparams *h,
                          float *params, float *grad, float *adam_m, float *adam_v, void *state, float *replicas_policy,
                          float *replicas_value, int32_t n_copies, void *ws, size_t ws_bytes, const void *epoch, void *stream)
{
    if (!epoch) return rover_internal_fail(ROVER_ERR_INVALID, "rover_ppo_apply_gated: epoch is NULL");
    if (reinterpret_cast<uintptr_t>(epoch) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "epoch must be 8-byte aligned");
    return apply_impl(policy, value, h, params, grad, adam_m, adam_v, state, replicas_policy, replicas_value, n_copies, ws, ws_bytes,
                      static_cast<const rover_ppo_epoch *>(epoch), stream);
}

int rover_ppo_epoch_end(const rover_ppo_hparams *h, const float *stats, int32_t n_minibatches, void *state, void *epoch,
                        int32_t schedule, float *kl_out, void *stream)
{
    if (!h || !stats || !state || !epoch) return rover_internal_fail(ROVER_ERR_INVALID, "rover_ppo_epoch_end: NULL argument");
    if (n_minibatches < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n_minibatches must be >= 1");
    if (schedule != 0 && schedule != 1) return rover_internal_fail(ROVER_ERR_INVALID, "schedule must be 0 or 1");
    if ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(epoch)) & 7)
        return rover_internal_fail(ROVER_ERR_INVALID, "state and epoch must be 8-byte aligned");
    int dev;
    if (int rc = device_of(stats, &dev)) return rc;
    DeviceGuard guard(dev);
    hipLaunchKernelGGL(ppo_epoch_end_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), stats, (int)n_minibatches,
                       h->kl_threshold, h->lr_factor, h->lr_min, h->lr_max, static_cast<rover_ppo_state *>(state),
                       static_cast<rover_ppo_epoch *>(epoch), (int)schedule, kl_out);
    return launched("ppo_epoch_end_kernel launch: %s");
}

int rover_ppo_gae(const rover_ppo_hparams *h, const float *rew, const float *done, const float *val, const float *last_v,
                  int32_t T, int32_t n_envs, float *adv, float *ret, void *stream)
{
    if (!h || !rew || !done || !val || !last_v || !adv || !ret) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (T < 1 || n_envs < 1) return rover_internal_fail(ROVER_ERR_INVALID, "T and n_envs must be >= 1");
    int dev;
    if (int rc = device_of(rew, &dev)) return rc;
    DeviceGuard guard(dev);
    const float gamma = h->gamma, gl = (float)((double)h->gamma * (double)h->lam);
    hipLaunchKernelGGL(ppo_gae_kernel, dim3(cdiv(n_envs, FT)), dim3(FT), 0, static_cast<hipStream_t>(stream), rew, done, val, last_v,
                       (int)T, (int)n_envs, gamma, gl, adv, ret);
    return launched("ppo_gae_kernel launch: %s");
}

int rover_ppo_kl_schedule(const rover_ppo_hparams *h, const float *stats, int32_t n_minibatches, void *state, float *kl_out,
                          void *stream)
{
    if (!h || !stats || !state) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (n_minibatches < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n_minibatches must be >= 1");
    int dev;
    if (int rc = device_of(stats, &dev)) return rc;
    DeviceGuard guard(dev);
    hipLaunchKernelGGL(ppo_kl_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), stats, (int)n_minibatches, h->kl_threshold,
                       h->lr_factor, h->lr_min, h->lr_max, static_cast<rover_ppo_state *>(state), kl_out);
    return launched("ppo_kl_kernel launch: %s");
}

int rover_policy_unpack(const rover_policy_desc *d, const float *packed, float *const *weights, float *const *biases)
{
    if (!d || !packed || !weights || !biases) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    const int nl = d->n_enc + d->n_mlp;
    if (d->n_enc < 0 || d->n_mlp < 1 || nl > ROVER_POLICY_MAX_LAYERS) return rover_internal_fail(ROVER_ERR_INVALID, "bad layer counts");
    for (int li = 0; li < nl; ++li) {
        const rover_policy_layer &l = d->layers[li];
        if (l.K < 1 || l.N < 1) return rover_internal_fail(ROVER_ERR_INVALID, "bad layer shape");
        if (!weights[li] || !biases[li]) return rover_internal_fail(ROVER_ERR_INVALID, "layer weight / bias is NULL");
        const int G = cdiv(l.K, 16);
        const float *w = packed + l.w_off;
        for (int nn = 0; nn < l.N; ++nn)
            for (int k = 0; k < l.K; ++k)
                weights[li][(size_t)nn * l.K + k] =
                    w[((((size_t)(nn >> 4) * G + (k >> 4)) * 64 + (nn & 15) + 16 * (k & 3)) << 2) + ((k >> 2) & 3)];
        for (int nn = 0; nn < l.N; ++nn) biases[li][nn] = packed[l.b_off + nn];
    }
    return ROVER_OK;
}

}  // extern "C"
