// sac_kernels.hip -- fused SAC update of the rover's Gaussian actor, twin critics and entropy coefficient (gfx950 / CDNA4,
// wave64).
//
// skrl SAC._update for the reference's tanh actor with a state-independent log_std and the Q(s, a) critic; see
// include/rover_sac.h for the contract and the reduction order.  The networks' forward, backward and weight gradients, the
// gather of the sampled rows, Adam and Polyak are offpolicy_net.hpp's, shared with td3_kernels.hip.  This file adds the
// one-thread-per-row heads (the Gaussian sample and its log-probability, y, the min of the critics, the Gaussian head's
// closed-form backward), their fixed-order reductions into the device state, the tail's Adam, the workspace and the entry points.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_hip.h"
#include "../../include/rover_policy.h"
#include "../../include/rover_sac.h"
#include "rover_internal.hpp"
#include "offpolicy_net.hpp"
#include "train_math.hpp"

namespace {

using State = rover_sac_state;
constexpr int NSUM = 5;                                      // per-row sums of the critic head
constexpr int NPSUM = 4;                                     // ... of the policy head: loss, logp, dL/dls (2)
constexpr int HD = 8;                                        // Gaussian head's per-row record: u (2), mu (2), t (2), p (2)
constexpr int GP = 4;                                        // dL/du per row: critic_1's (2), critic_2's (2)
constexpr int TAIL = 8;                                      // log_std (2 + 2 pad), log_alpha (1 + 3 pad)
constexpr float LS_MIN = -20.0f, LS_MAX = 2.0f, U_MIN = -1.0f, U_MAX = 1.0f;
constexpr float HALF_LN_2PI = 0.91893853320467274178f;

// the entropy coefficient from the parameter vector's log_alpha
__device__ __forceinline__ float alpha_of(const float *log_alpha) { return (float)exp((double)log_alpha[0]); }

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
// critics' backward,
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

// the tail: log_std (floats 0 .. 3) with the policy's scalars, log_alpha (floats 4 .. 7) with the entropy step's, if it is learned
__global__ __launch_bounds__(64) void sac_tail_adam_kernel(float *params, const float *grad, float *m, float *v, const float *sc_actor,
                                                           const float *sc_entropy, int learn_entropy, float beta1, float beta2, float eps)
{
    const int e = threadIdx.x;
    if (e >= TAIL) return;
    if (e >= 4 && !learn_entropy) return;
    const float *sc = e < 4 ? sc_actor : sc_entropy;
    adam_element(params, m, v, e, grad[e], sc, sc + 1, beta1, beta2, eps);
}

// ---- host side
size_t tail_off() { return net_floats(false) + 2 * net_floats(true); }
size_t param_floats() { return (tail_off() + TAIL + 63) & ~(size_t)63; }

int check_nets(const rover_policy_desc *actor, const rover_policy_desc *critic)
{
    if (!actor || !critic) return rover_internal_fail(ROVER_ERR_INVALID, "descriptor is NULL");
    if (!is_net(actor, false, ROVER_ACT_TANH, true) || !is_net(critic, true, ROVER_ACT_NONE, true))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "the fused SAC update runs the reference's tanh actor (rover_policy_default_desc(2, 1), "
                                                          "packed by rover_policy_pack) and the Q(s, a) critic (rover_td3_critic_desc, "
                                                          "packed by rover_td3_critic_pack) only");
    return ROVER_OK;
}

// workspace layout: per-row vectors (ro_s, ro_n as int64; a (2), r, nt, y / min q, logp, the Gaussian head's record (HD), the
// critics' dL/du (GP) as float), row partials, then 5 network regions (cache + scratch, ROW_F floats per row each): 0 actor,
// 1 / 2 target critics, 3 / 4 critics; then the weight-gradient chunk partials of both critics
constexpr int NREG = 5;
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

// the actor on the ring rows `ro` and its Gaussian head on eps[:, ecol .. ecol + 2): u, mu, t, p into w.hd, logp into w.logp
int act(const Ws &w, Region *reg, const Net &pi, const float *tail, const int64_t *ro, const float *obs, const float *eps, int ecol,
        int n, hipStream_t s)
{
    FwdJob ja = {pi, ro, nullptr, 0, reg};
    if (int rc = forward<State>(&ja, 1, obs, n, s)) return rc;
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
    if (!is_net(actor, false, ROVER_ACT_TANH, true) || !is_net(critic, true, ROVER_ACT_NONE, true)) return 0;
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
    if (int rc = forward<State>(jc, 4, obs_ring, n, s)) return rc;
    CriticHead H = {};
    H.tq1 = w.reg[1].cache[NL - 1]; H.tq2 = w.reg[2].cache[NL - 1]; H.q1 = w.reg[3].cache[NL - 1]; H.q2 = w.reg[4].cache[NL - 1];
    H.r = w.r; H.nt = w.nt; H.logp = w.logp; H.log_alpha = tail + 4; H.gamma = h->gamma; H.inv_n = 1.0f / (float)n;
    H.dz1 = w.reg[3].scr[NL - 1]; H.dz2 = w.reg[4].scr[NL - 1];
    H.y_out = y_out; H.rows = n; H.rowp = w.rowp;
    hipLaunchKernelGGL(sac_critic_head_kernel, dim3(cdiv(n, FT)), dim3(FT), 0, s, H);
    hipLaunchKernelGGL(sac_critic_final_kernel, dim3(1), dim3(FT), 0, s, (const float *)w.rowp, cdiv(n, FT), H.inv_n, h->beta1, h->beta2,
                       h->critic_lr, st);
    if (int rc = launched("sac critic head launch: %s")) return rc;
    // backward of both critics, weight gradients into the critic blocks, Adam over both
    const Net qs[2] = {q1, q2};
    Region *regs[2] = {&w.reg[3], &w.reg[4]};
    for (int l = NL - 1; l >= 1; --l)
        if (int rc = back_layer<State>(qs, regs, 2, l, n, s)) return rc;
    if (int rc = wgrad<State>(qs, regs, w.ro_s, 2, obs_ring, n, w.part, grad + Pa, s)) return rc;
    hipLaunchKernelGGL(offpolicy_adam_kernel<State>, dim3(cdiv((int)(2 * Pc), FT)), dim3(FT), 0, s, params + Pa, (const float *)grad + Pa,
                       adam_m + Pa, adam_v + Pa, (const float *)&st->critic_step_size, (int)(2 * Pc), h->beta1, h->beta2, h->eps,
                       (float *)nullptr, 0);
    return launched("offpolicy_adam_kernel launch: %s");
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
    if (int rc = forward<State>(jq, 2, obs_ring, n, s)) return rc;
    hipLaunchKernelGGL(sac_min_head_kernel, dim3(cdiv(n, FT)), dim3(FT), 0, s, (const float *)w.reg[3].cache[NL - 1],
                       (const float *)w.reg[4].cache[NL - 1], w.reg[3].scr[NL - 1], w.reg[4].scr[NL - 1], w.y, inv_n, n);
    if (int rc = launched("sac_min_head_kernel launch: %s")) return rc;
    // both critics' MLP backward down to their input M, then only the two action columns: critic k's dL/du into g[:, 2 k .. 2 k + 2)
    const Net qs[2] = {q1, q2};
    Region *regs[2] = {&w.reg[3], &w.reg[4]};
    for (int l = NL - 1; l >= 3; --l)
        if (int rc = back_layer<State>(qs, regs, 2, l, n, s)) return rc;
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
        hipLaunchKernelGGL(offpolicy_back_kernel<State>, dim3(cdiv(n, 64), 1, 2), dim3(FT), 0, s, L);
        if (int rc = launched("offpolicy_back_kernel launch: %s")) return rc;
    }
    GaussBack B = {};
    B.hd = w.hd; B.logp = w.logp; B.minq = w.y; B.g = w.g; B.log_std = tail; B.log_alpha = tail + 4; B.eps = eps; B.ecol = 2;
    B.inv_n = inv_n; B.dz6 = RA.scr[NL - 1]; B.u_out = u_out; B.logp_out = logp_out; B.dmean_out = dmean_out; B.rows = n;
    B.rowp = w.rowp;
    hipLaunchKernelGGL(sac_gauss_back_kernel, dim3(cdiv(n, FT)), dim3(FT), 0, s, B);
    if (int rc = launched("sac_gauss_back_kernel launch: %s")) return rc;
    // the actor's backward and weight gradients into the actor block
    Region *ra[1] = {&RA};
    for (int l = NL - 1; l >= 1; --l)
        if (int rc = back_layer<State>(&pi, ra, 1, l, n, s)) return rc;
    if (int rc = wgrad<State>(&pi, ra, w.ro_s, 1, obs_ring, n, w.part, grad, s)) return rc;
    PolicyFinal F = {};
    F.rowp = w.rowp; F.nblk = cdiv(n, FT); F.inv_n = inv_n; F.beta1 = h->beta1; F.beta2 = h->beta2; F.actor_lr = h->actor_lr;
    F.entropy_lr = h->entropy_lr; F.target_entropy = h->target_entropy; F.learn_entropy = h->learn_entropy != 0;
    F.tail_p = tail; F.tail_g = grad + To; F.tail_n = (int)(param_floats() - To); F.st = st;
    hipLaunchKernelGGL(sac_policy_final_kernel, dim3(1), dim3(FT), 0, s, F);
    if (int rc = launched("sac_policy_final_kernel launch: %s")) return rc;
    hipLaunchKernelGGL(offpolicy_adam_kernel<State>, dim3(cdiv((int)Pa, FT)), dim3(FT), 0, s, params, (const float *)grad, adam_m, adam_v,
                       (const float *)&st->actor_step_size, (int)Pa, h->beta1, h->beta2, h->eps, replicas_actor, (int)n_copies);
    hipLaunchKernelGGL(sac_tail_adam_kernel, dim3(1), dim3(64), 0, s, params + To, (const float *)grad + To, adam_m + To, adam_v + To,
                       (const float *)&st->actor_step_size, (const float *)&st->entropy_step_size, F.learn_entropy, h->beta1, h->beta2,
                       h->eps);
    return launched("offpolicy_adam_kernel launch: %s");
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
    hipLaunchKernelGGL(offpolicy_polyak_kernel<State>, dim3((unsigned)((count + FT - 1) / FT)), dim3(FT), 0,
                       static_cast<hipStream_t>(stream), target, params + net_floats(false), count, keep, h->polyak);
    return launched("offpolicy_polyak_kernel launch: %s");
}

}  // extern "C"
