// offpolicy_net.hpp -- the network machinery of the off-policy updates (td3_kernels.hip, sac_kernels.hip): the reference actor and
// the Q(s, a) critic layer by layer over the sampled rows, every dense product on v_mfma_f32_16x16x4_f32, in the pattern of
// trpo_kernels.hip (adapted here; that file is not shared):
//   offpolicy_dense_kernel    Z = A W^T + b, act(Z) for up to 4 networks per launch (blockIdx.z): one wave per 16 rows x 64
//                             columns; the packed weights are the B fragments as they lie (one float4 per lane per 16 k).  Layer 2
//                             also writes the MLP input's proprioceptive columns and, for a critic, its two action columns;
//   offpolicy_back_kernel     backward dA = dZ W (times LeakyReLU' of the stored activation, or not: the action columns), up to 2
//                             networks per launch;
//   offpolicy_wgrad_kernel    dW = dZ^T A and db = sum dZ per (16 x 16 tile, 512-row chunk) over up to 12 layers (both critics)
//                             in the packed layout;
//   offpolicy_combine_kernel  the chunk partials added in chunk order;
// plus the gather of the sampled rows from the observation ring, the fixed-order reductions the trainers' final kernels use,
// Adam (train_shared.hpp's element and scalars) and Polyak, and the host side that lays the networks out and launches them.
//
// Both trainers include this one text; what differs between them (the heads, the final kernels, the workspace, the argument
// checks, the entry points) stays in their files.  Every kernel is a template on the trainer's device state struct
// (rover_td3_state, rover_sac_state): the gather kernel stores its bad_index word there, and the two trainers' kernels keep
// different names (offpolicy_dense_kernel<rover_sac_state>) in a trace and in the library.  The launchers take the same struct
// as their template argument.
#ifndef ROVER_OFFPOLICY_NET_HPP
#define ROVER_OFFPOLICY_NET_HPP

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/rover_hip.h"
#include "../../include/rover_policy.h"
#include "rover_internal.hpp"
#include "train_shared.hpp"

namespace {

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
constexpr int RP = 8;                                        // stride of a block's partials

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

// ---- gather: the ring rows of s and s' (64-bit row numbers) and the stored transition of every sampled row
template <class State>
struct GatherArgs {
    const int64_t *idx; int n; int64_t valid;
    int num_envs, slots;
    const int32_t *pos;
    const float *act, *rew; const uint8_t *term;     // NULL for the actor / policy step
    int64_t *ro_s, *ro_n;
    float *a, *r, *nt;
    State *st;
};
template <class State>
__global__ __launch_bounds__(FT) void offpolicy_gather_kernel(GatherArgs<State> A)
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
template <class State>
__global__ __launch_bounds__(FT) void offpolicy_dense_kernel(DenseLaunch L)
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

// ---- backward: out[r][k - ocol] = (sum_n dZ[r][n] W[n][k]) * LeakyReLU'(aref[r][k]) (aref NULL: no derivative) for k in
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
template <class State>
__global__ __launch_bounds__(FT) void offpolicy_back_kernel(BackLaunch L)
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
template <class State>
__global__ __launch_bounds__(FT) void offpolicy_wgrad_kernel(WgradArgs A)
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
template <class State>
__global__ __launch_bounds__(FT) void offpolicy_combine_kernel(const float *part, int nch, int P, float *out)
{
    const int e = blockIdx.x * FT + threadIdx.x;
    if (e >= P) return;
    float s = part[e];
    for (int c = 1; c < nch; ++c) s += part[(size_t)c * P + e];
    out[e] = s;
}

// ---- for the trainers' final kernels (one workgroup each)
// thread t adds partials t, t + 256, ... in order, then the tree; total of row-term i in tot[i] (every thread)
__device__ void reduce_rows(const float *rowp, int nblk, int nterms, float *tot, float *red)
{
    for (int i = 0; i < nterms; ++i) {
        float s = 0.0f;
        for (int b = threadIdx.x; b < nblk; b += FT) s += rowp[(size_t)b * RP + i];
        tot[i] = block_sum(s, red);
    }
}

// ---- Adam (train_shared.hpp's element, no clipping) over P floats; sc = {step_size, bc2_sqrt} in the state; then the replicas
template <class State>
__global__ __launch_bounds__(FT) void offpolicy_adam_kernel(float *params, const float *grad, float *m, float *v, const float *sc, int P,
                                                            float beta1, float beta2, float eps, float *rep, int n_copies)
{
    const int e = blockIdx.x * FT + threadIdx.x;
    if (e >= P) return;
    const float p = adam_element(params, m, v, e, grad[e], sc, sc + 1, beta1, beta2, eps);
    refresh_replicas(rep, n_copies, P, e, p);
}

// ---- Polyak: t.mul_(1 - tau); t.add_(tau * p) -- two fp32 roundings per product, one per sum (no contraction)
template <class State>
__global__ __launch_bounds__(FT) void offpolicy_polyak_kernel(float *t, const float *p, size_t count, float keep, float tau)
{
    const size_t e = (size_t)blockIdx.x * FT + threadIdx.x;
    if (e >= count) return;
    const float a = t[e] * keep;
    const float b = p[e] * tau;
    t[e] = a + b;
}

// ---- host side
int out_of(int l, bool critic) { return l < NL - 1 ? LN[l] : (critic ? 1 : 2); }
int in_of(int l, bool critic) { return critic ? CK[l] : AK[l]; }
size_t net_floats(bool critic)
{
    size_t n = 0;
    for (int l = 0; l < NL; ++l) n += layer_weight_floats(out_of(l, critic), in_of(l, critic)) + layer_bias_floats(out_of(l, critic));
    return n;
}

// the shapes (and, with `packed`, the offsets the pack sets) of the actor / the critic with layer 6's activation last_act
bool is_net(const rover_policy_desc *d, bool critic, int last_act, bool packed)
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
        if (l.act != (i < NL - 1 ? ROVER_ACT_LEAKY_RELU : last_act)) return false;
        if ((l.split_k != 0) != (i == 0 || i == NL - 1)) return false;
        if (packed && l.w_off != off) return false;
        off += layer_weight_floats(N, K);
        if (packed && l.b_off != off) return false;
        off += layer_bias_floats(N);
    }
    return true;
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

// one network's region of a trainer's workspace: cache (the layer outputs) and scratch (their dZ), ROW_F floats per row each
struct Region {
    float *cache[NL], *scr[NL];
};
size_t rowp_floats(int rows) { return al4((size_t)RP * cdiv(rows, FT)); }
size_t part_floats(int rows) { return (size_t)cdiv(rows, CH) * (2 * net_floats(true)); }   // the chunk partials of both critics

// the forward of up to MAXZ networks over `rows` rows; net z reads observation rows ro[z] and (critics) actions ain[z] (any
// pitch aip) and writes its layer outputs to reg[z]->cache.  The last layer has no activation: a tanh actor's head applies it.
struct FwdJob {
    Net net;
    const int64_t *ro;
    const float *ain; int aip;
    Region *reg;
};
template <class State>
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
        hipLaunchKernelGGL(offpolicy_dense_kernel<State>, dim3(cdiv(rows, 64), cdiv(N, 64), nz), dim3(FT), 0, s, L);
        if (int rc = launched("offpolicy_dense_kernel launch: %s")) return rc;
    }
    return ROVER_OK;
}

// backward of layer l for nz networks at once: dZ_{l-1} = (dZ_l W_l) * LeakyReLU'(a_{l-1}) into scr[l - 1]
template <class State>
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
    hipLaunchKernelGGL(offpolicy_back_kernel<State>, dim3(cdiv(rows, 64), cdiv(nk, 64), nz), dim3(FT), 0, s, L);
    return launched("offpolicy_back_kernel launch: %s");
}

// weight gradients of nz networks whose packed blocks lie back to back (block_floats each) into out[0 .. nz * block_floats)
template <class State>
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
    hipLaunchKernelGGL(offpolicy_wgrad_kernel<State>, dim3(cdiv(W.jobs[j], 4), nch), dim3(FT), 0, s, W);
    if (int rc = launched("offpolicy_wgrad_kernel launch: %s")) return rc;
    hipLaunchKernelGGL(offpolicy_combine_kernel<State>, dim3(cdiv(W.P, FT)), dim3(FT), 0, s, (const float *)part, nch, W.P, out);
    return launched("offpolicy_combine_kernel launch: %s");
}

// the gather into a trainer's workspace (its Ws: ro_s, ro_n, a, r, nt); act, rew, term NULL for the actor / policy step
template <class Ws, class State>
int gather(const Ws &w, const int64_t *idx, int n, int64_t valid, int num_envs, int slots, const int32_t *pos, const float *act,
           const float *rew, const uint8_t *term, State *st, hipStream_t s)
{
    GatherArgs<State> G = {};
    G.idx = idx; G.n = n; G.valid = valid; G.num_envs = num_envs; G.slots = slots; G.pos = pos;
    G.act = act; G.rew = rew; G.term = term;
    G.ro_s = w.ro_s; G.ro_n = w.ro_n; G.a = w.a; G.r = w.r; G.nt = w.nt; G.st = st;
    hipLaunchKernelGGL(offpolicy_gather_kernel<State>, dim3(cdiv(n, FT)), dim3(FT), 0, s, G);
    return launched("offpolicy_gather_kernel launch: %s");
}

}  // namespace

#endif  // ROVER_OFFPOLICY_NET_HPP
