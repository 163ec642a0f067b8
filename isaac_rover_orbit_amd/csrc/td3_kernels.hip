// td3_kernels.hip -- fused TD3 update of the rover's actor and twin critics (gfx950 / CDNA4, wave64).
//
// skrl TD3._update for the reference actor and the Q(s, a) critic; see include/rover_td3.h for the contract and the
// reduction order.  The networks' forward, backward and weight gradients, the gather of the sampled rows, Adam and Polyak are
// offpolicy_net.hpp's, shared with sac_kernels.hip.  This file adds the smoothing of the target action, the one-thread-per-row
// heads (y, loss gradients), their fixed-order reductions into the device state, the workspace and the entry points.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_hip.h"
#include "../../include/rover_policy.h"
#include "../../include/rover_td3.h"
#include "rover_internal.hpp"
#include "offpolicy_net.hpp"
#include "train_math.hpp"

namespace {

using State = rover_td3_state;
constexpr int NSUM = 5;                                      // per-row sums of the critic head

// ---- smoothing of the target action (in place, pitch 4): clamp(a' + clamp(noise, -clip, clip), lo, hi)
__global__ __launch_bounds__(FT) void td3_smooth_kernel(float *a, const float *noise, int n, float clip, float lo, float hi)
{
    const int r = blockIdx.x * FT + threadIdx.x;
    if (r >= n) return;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float z = fminf(fmaxf(noise[2 * (size_t)r + c], -clip), clip);
        a[(size_t)r * MW[NL - 1] + c] = fminf(fmaxf(a[(size_t)r * MW[NL - 1] + c] + z, lo), hi);
    }
}

// ---- critic head: y, the per-row squared errors and the critics' dZ6; block partials (fixed tree) to rowp[block * RP + i]
struct CriticHead {
    const float *tq1, *tq2, *q1, *q2;   // last-layer outputs, pitch 4
    const float *r, *nt;
    float gamma, inv_n;
    float *dz1, *dz2;                   // dZ6 of critic_1 / critic_2, pitch 4
    float *y_out;
    int rows;
    float *rowp;
};
__global__ __launch_bounds__(FT) void td3_critic_head_kernel(CriticHead A)
{
    __shared__ float red[FT];
    const int r = blockIdx.x * FT + threadIdx.x;
    float t[NSUM] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (r < A.rows) {
        const size_t o = (size_t)r * MW[NL - 1];
        const float mq = tmin(A.tq1[o], A.tq2[o]);
        const float y = A.r[r] + (A.gamma * A.nt[r]) * mq;     // rewards + gamma * !terminated * min(tq1, tq2)
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
// ---- actor head: dZ6 of critic_1 = d(-mean q1)/dq1 = -1/B, the sum of q1 to rowp
__global__ __launch_bounds__(FT) void td3_actor_head_kernel(const float *q, float *dz, float inv_n, int rows, float *rowp)
{
    __shared__ float red[FT];
    const int r = blockIdx.x * FT + threadIdx.x;
    float v = 0.0f;
    if (r < rows) {
        v = q[(size_t)r * MW[NL - 1]];
        dz[(size_t)r * MW[NL - 1]] = -inv_n;
    }
    const float tot = block_sum(v, red);
    if (threadIdx.x == 0) rowp[(size_t)blockIdx.x * RP] = tot;
}

__global__ __launch_bounds__(FT) void td3_critic_final_kernel(const float *rowp, int nblk, float inv_n, float beta1, float beta2, float lr,
                                                              rover_td3_state *st)
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
        st->critic_updates += 1;
        adam_scalars(st->critic_step, beta1, beta2, lr, &st->critic_step_size, &st->critic_bc2_sqrt);
    }
}
__global__ __launch_bounds__(FT) void td3_actor_final_kernel(const float *rowp, int nblk, float inv_n, float beta1, float beta2, float lr,
                                                             rover_td3_state *st)
{
    __shared__ float red[FT];
    float tot[1];
    reduce_rows(rowp, nblk, 1, tot, red);
    if (threadIdx.x == 0) {
        st->policy_loss = -(tot[0] * inv_n);
        st->actor_step += 1;
        adam_scalars(st->actor_step, beta1, beta2, lr, &st->actor_step_size, &st->actor_bc2_sqrt);
    }
}

// ---- host side
size_t param_floats() { return (net_floats(false) + 2 * net_floats(true) + 63) & ~(size_t)63; }

int check_nets(const rover_policy_desc *actor, const rover_policy_desc *critic)
{
    if (!actor || !critic) return rover_internal_fail(ROVER_ERR_INVALID, "descriptor is NULL");
    if (!is_net(actor, false, ROVER_ACT_NONE, true) || !is_net(critic, true, ROVER_ACT_NONE, true))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "the fused TD3 update runs the reference actor (rover_policy_default_desc(2, 0), "
                                                          "packed by rover_policy_pack) and the Q(s, a) critic (rover_td3_critic_desc, "
                                                          "packed by rover_td3_critic_pack) only");
    return ROVER_OK;
}

// workspace layout: per-row vectors (ro_s, ro_n as int64; a (2), r, nt, y as float), row partials, then 5 network regions
// (cache + scratch, ROW_F floats per row each): 0 actor / target actor, 1 / 2 target critics, 3 / 4 critics; then the
// weight-gradient chunk partials of both critics
constexpr int NREG = 5;
size_t ws_bytes_for(int rows)
{
    const size_t R = (size_t)rows;
    size_t f = 4 * al4(R) /* ro_s, ro_n: 2 floats each */ + 2 * al4(R) + 3 * al4(R) + rowp_floats(rows) + NREG * 2 * (size_t)ROW_F * R +
               part_floats(rows);
    return sizeof(float) * f;
}
struct Ws {
    int64_t *ro_s, *ro_n;
    float *a, *r, *nt, *y, *rowp, *part;
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

int common_checks(const rover_policy_desc *actor, const rover_policy_desc *critic, const rover_td3_hparams *h, const void *params,
                  const void *grad, const void *adam_m, const void *adam_v, const float *obs_ring, int32_t slots, int32_t num_envs,
                  const int32_t *ring_pos, const int64_t *idx, int32_t n, int64_t valid_rows, const void *ws, size_t ws_bytes,
                  const void *state)
{
    if (int rc = check_nets(actor, critic)) return rc;
    if (!h || !params || !grad || !adam_m || !adam_v || !obs_ring || !ring_pos || !idx || !ws || !state)
        return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (n < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n must be >= 1");
    if (slots < 2 || num_envs < 1) return rover_internal_fail(ROVER_ERR_INVALID, "the ring needs >= 2 slots and >= 1 env");
    if (valid_rows < 1 || valid_rows > (int64_t)(slots - 1) * num_envs)
        return rover_internal_fail(ROVER_ERR_INVALID, "valid_rows must be in [1, (slots - 1) * num_envs]");
    if (ws_bytes < rover_td3_workspace_bytes(n)) return rover_internal_fail(ROVER_ERR_INVALID, "TD3 workspace too small");
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grad) |
         reinterpret_cast<uintptr_t>(adam_m) | reinterpret_cast<uintptr_t>(adam_v)) & 15)
        return rover_internal_fail(ROVER_ERR_INVALID, "workspace and parameter vectors must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(state) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "state must be 8-byte aligned");
    return ROVER_OK;
}

}  // namespace

extern "C" {

int rover_td3_default_hparams(rover_td3_hparams *h)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "hparams is NULL");
    h->gamma = 0.99f;
    h->polyak = 0.005f;
    h->actor_lr = 1e-4f; h->critic_lr = 1e-4f;
    h->beta1 = 0.9f; h->beta2 = 0.999f; h->eps = 1e-8f;
    h->noise_clip = 0.5f;
    h->act_min = -1.0f; h->act_max = 1.0f;
    return ROVER_OK;
}
size_t rover_td3_hparams_bytes(void) { return sizeof(rover_td3_hparams); }
size_t rover_td3_state_bytes(void) { return sizeof(rover_td3_state); }

int rover_td3_critic_desc(rover_policy_desc *d)
{
    if (!d) return rover_internal_fail(ROVER_ERR_INVALID, "desc is NULL");
    memset(d, 0, sizeof(*d));
    d->obs_dim = OBS; d->prop_dim = PROP; d->enc_offset = ENC_OFF; d->enc_dim = CK[0];
    d->n_enc = 2; d->n_mlp = 4; d->leaky_slope = 0.01f;
    for (int i = 0; i < NL; ++i) {
        d->layers[i].K = CK[i]; d->layers[i].N = out_of(i, true);
        d->layers[i].act = i < NL - 1 ? ROVER_ACT_LEAKY_RELU : ROVER_ACT_NONE;
        d->layers[i].split_k = (i == 0 || i == NL - 1) ? 1 : 0;   // as rover_policy_default_desc
    }
    return ROVER_OK;
}

int rover_td3_critic_pack(rover_policy_desc *d, const float *const *weights, const float *const *biases, float *packed)
{
    if (!d || !weights || !biases || !packed) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (!is_net(d, true, ROVER_ACT_NONE, false))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "not the TD3 critic layout (rover_td3_critic_desc)");
    size_t off = 0;
    for (int li = 0; li < NL; ++li) {
        rover_policy_layer &l = d->layers[li];
        if (!weights[li] || !biases[li]) return rover_internal_fail(ROVER_ERR_INVALID, "layer weight / bias is NULL");
        const int G = cdiv(l.K, 16), T = cdiv(l.N, 16);
        l.w_off = (uint32_t)off;
        float *w = packed + off;
        for (int t = 0; t < T; ++t)
            for (int g = 0; g < G; ++g)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j) {
                        const int nn = 16 * t + (lane & 15), k = 16 * g + 4 * j + (lane >> 4);
                        w[(((size_t)t * G + g) * 64 + lane) * 4 + j] = (nn < l.N && k < l.K) ? weights[li][(size_t)nn * l.K + k] : 0.0f;
                    }
        off += layer_weight_floats(l.N, l.K);
        l.b_off = (uint32_t)off;
        for (size_t i = 0; i < layer_bias_floats(l.N); ++i) packed[off + i] = i < (size_t)l.N ? biases[li][i] : 0.0f;
        off += layer_bias_floats(l.N);
    }
    return ROVER_OK;
}

size_t rover_td3_param_floats(const rover_policy_desc *actor, const rover_policy_desc *critic)
{
    if (!is_net(actor, false, ROVER_ACT_NONE, true) || !is_net(critic, true, ROVER_ACT_NONE, true)) return 0;
    return param_floats();
}
size_t rover_td3_workspace_bytes(int32_t max_rows) { return max_rows > 0 ? ws_bytes_for(max_rows) : 0; }

int rover_td3_critic_step(const rover_policy_desc *actor, const rover_policy_desc *critic, const rover_td3_hparams *h,
                          float *params, const float *target, float *grad, float *adam_m, float *adam_v, const float *obs_ring,
                          int32_t slots, int32_t num_envs, const int32_t *ring_pos, const float *act, const float *rew,
                          const uint8_t *terminated, const int64_t *idx, int32_t n, int64_t valid_rows, const float *noise,
                          void *ws, size_t ws_bytes, void *state, float *y_out, void *stream)
{
    if (int rc = common_checks(actor, critic, h, params, grad, adam_m, adam_v, obs_ring, slots, num_envs, ring_pos, idx, n, valid_rows,
                               ws, ws_bytes, state))
        return rc;
    if (!target || !act || !rew || !terminated) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (reinterpret_cast<uintptr_t>(target) & 15) return rover_internal_fail(ROVER_ERR_INVALID, "target must be 16-byte aligned");
    int dev;
    if (int rc = device_of(params, &dev)) return rc;
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    rover_td3_state *st = static_cast<rover_td3_state *>(state);
    Ws w = ws_at(ws, n);
    const size_t Pa = net_floats(false), Pc = net_floats(true);
    const Net tpi = net_at(actor, target, false);
    const Net tq1 = net_at(critic, target + Pa, true), tq2 = net_at(critic, target + Pa + Pc, true);
    const Net q1 = net_at(critic, params + Pa, true), q2 = net_at(critic, params + Pa + Pc, true);
    if (int rc = gather(w, idx, n, valid_rows, num_envs, slots, ring_pos, act, rew, terminated, st, s)) return rc;
    // a' = target_policy(s') [smoothed]
    FwdJob ja = {tpi, w.ro_n, nullptr, 0, &w.reg[0]};
    if (int rc = forward<State>(&ja, 1, obs_ring, n, s)) return rc;
    float *a_next = w.reg[0].cache[NL - 1];
    if (noise) {
        hipLaunchKernelGGL(td3_smooth_kernel, dim3(cdiv(n, FT)), dim3(FT), 0, s, a_next, noise, n, h->noise_clip, h->act_min, h->act_max);
        if (int rc = launched("td3_smooth_kernel launch: %s")) return rc;
    }
    // target critics on (s', a') and critics on (s, a) in the same launches
    FwdJob jc[4] = {{tq1, w.ro_n, a_next, MW[NL - 1], &w.reg[1]}, {tq2, w.ro_n, a_next, MW[NL - 1], &w.reg[2]},
                    {q1, w.ro_s, w.a, 2, &w.reg[3]}, {q2, w.ro_s, w.a, 2, &w.reg[4]}};
    if (int rc = forward<State>(jc, 4, obs_ring, n, s)) return rc;
    CriticHead H = {};
    H.tq1 = w.reg[1].cache[NL - 1]; H.tq2 = w.reg[2].cache[NL - 1]; H.q1 = w.reg[3].cache[NL - 1]; H.q2 = w.reg[4].cache[NL - 1];
    H.r = w.r; H.nt = w.nt; H.gamma = h->gamma; H.inv_n = 1.0f / (float)n;
    H.dz1 = w.reg[3].scr[NL - 1]; H.dz2 = w.reg[4].scr[NL - 1];
    H.y_out = y_out; H.rows = n; H.rowp = w.rowp;
    hipLaunchKernelGGL(td3_critic_head_kernel, dim3(cdiv(n, FT)), dim3(FT), 0, s, H);
    hipLaunchKernelGGL(td3_critic_final_kernel, dim3(1), dim3(FT), 0, s, (const float *)w.rowp, cdiv(n, FT), H.inv_n, h->beta1, h->beta2,
                       h->critic_lr, st);
    if (int rc = launched("td3 critic head launch: %s")) return rc;
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

int rover_td3_actor_step(const rover_policy_desc *actor, const rover_policy_desc *critic, const rover_td3_hparams *h,
                         float *params, float *grad, float *adam_m, float *adam_v, const float *obs_ring, int32_t slots,
                         int32_t num_envs, const int32_t *ring_pos, const int64_t *idx, int32_t n, int64_t valid_rows,
                         void *ws, size_t ws_bytes, void *state, float *replicas_actor, int32_t n_copies, float *dact_out,
                         void *stream)
{
    if (int rc = common_checks(actor, critic, h, params, grad, adam_m, adam_v, obs_ring, slots, num_envs, ring_pos, idx, n, valid_rows,
                               ws, ws_bytes, state))
        return rc;
    if (replicas_actor && n_copies < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n_copies must be >= 1");
    int dev;
    if (int rc = device_of(params, &dev)) return rc;
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    rover_td3_state *st = static_cast<rover_td3_state *>(state);
    Ws w = ws_at(ws, n);
    const size_t Pa = net_floats(false);
    const Net pi = net_at(actor, params, false), q1 = net_at(critic, params + Pa, true);
    Region &RA = w.reg[0], &RQ = w.reg[3];
    if (int rc = gather(w, idx, n, valid_rows, num_envs, slots, ring_pos, nullptr, nullptr, nullptr, st, s)) return rc;
    FwdJob ja = {pi, w.ro_s, nullptr, 0, &RA};
    if (int rc = forward<State>(&ja, 1, obs_ring, n, s)) return rc;
    FwdJob jq = {q1, w.ro_s, RA.cache[NL - 1], MW[NL - 1], &RQ};
    if (int rc = forward<State>(&jq, 1, obs_ring, n, s)) return rc;
    const float inv_n = 1.0f / (float)n;
    hipLaunchKernelGGL(td3_actor_head_kernel, dim3(cdiv(n, FT)), dim3(FT), 0, s, (const float *)RQ.cache[NL - 1], RQ.scr[NL - 1], inv_n, n,
                       w.rowp);
    hipLaunchKernelGGL(td3_actor_final_kernel, dim3(1), dim3(FT), 0, s, (const float *)w.rowp, cdiv(n, FT), inv_n, h->beta1, h->beta2,
                       h->actor_lr, st);
    if (int rc = launched("td3 actor head launch: %s")) return rc;
    // critic_1's MLP backward down to its input M, then only the two action columns: dL/da into the actor's dZ6
    Region *rq[1] = {&RQ};
    for (int l = NL - 1; l >= 3; --l)
        if (int rc = back_layer<State>(&q1, rq, 1, l, n, s)) return rc;
    {
        BackLaunch L = {};
        L.rows = n; L.slope = 0.01f;
        Back &B = L.d[0];
        B.dz = RQ.scr[2]; B.dzp = MW[2];
        B.W = q1.p + q1.w_off[2]; B.K = CK[2]; B.N = LN[2];
        B.aref = nullptr; B.arp = 0;
        B.out = RA.scr[NL - 1]; B.op = MW[NL - 1]; B.ocol = ACOL;
        B.k0 = ACOL; B.nk = 2;
        hipLaunchKernelGGL(offpolicy_back_kernel<State>, dim3(cdiv(n, 64), 1, 1), dim3(FT), 0, s, L);
        if (int rc = launched("offpolicy_back_kernel launch: %s")) return rc;
    }
    if (dact_out) {
        hipError_t e = hipMemcpy2DAsync(dact_out, 2 * sizeof(float), RA.scr[NL - 1], MW[NL - 1] * sizeof(float), 2 * sizeof(float), n,
                                        hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "dact copy: %s", hipGetErrorString(e));
    }
    Region *ra[1] = {&RA};
    for (int l = NL - 1; l >= 1; --l)
        if (int rc = back_layer<State>(&pi, ra, 1, l, n, s)) return rc;
    if (int rc = wgrad<State>(&pi, ra, w.ro_s, 1, obs_ring, n, w.part, grad, s)) return rc;
    hipLaunchKernelGGL(offpolicy_adam_kernel<State>, dim3(cdiv((int)Pa, FT)), dim3(FT), 0, s, params, (const float *)grad, adam_m, adam_v,
                       (const float *)&st->actor_step_size, (int)Pa, h->beta1, h->beta2, h->eps, replicas_actor, (int)n_copies);
    return launched("offpolicy_adam_kernel launch: %s");
}

int rover_td3_polyak(const rover_td3_hparams *h, float *target, const float *params, size_t count, void *stream)
{
    if (!h || !target || !params) return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (count == 0) return ROVER_OK;
    int dev;
    if (int rc = device_of(target, &dev)) return rc;
    DeviceGuard guard(dev);
    const float keep = (float)(1.0 - (double)h->polyak);
    hipLaunchKernelGGL(offpolicy_polyak_kernel<State>, dim3((unsigned)((count + FT - 1) / FT)), dim3(FT), 0,
                       static_cast<hipStream_t>(stream), target, params, count, keep, h->polyak);
    return launched("offpolicy_polyak_kernel launch: %s");
}

}  // extern "C"
