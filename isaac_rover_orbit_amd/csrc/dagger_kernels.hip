// dagger_kernels.hip -- fused DAgger update of the depth student (gfx950 / CDNA4, wave64).
//
// One supervised step of the reference's policy network on student rows against the teacher's labels; see include/rover_dagger.h
// for the contract and the reduction order.  The network's forward, backward and weight gradients and the gather of the sampled
// rows are offpolicy_net.hpp's, shared with td3_kernels.hip and sac_kernels.hip, under this trainer's state type.  This file adds
// the imitation loss head with its closed-form tanh backward, the gradient's norm, the final reduce into the device state, Adam
// with clip_grad_norm_'s coefficient (train_shared.hpp), the workspace and the entry point.  The collector's kernels are
// dagger_collect_kernels.hip's: offpolicy_net.hpp and td3_actor_tile.hpp give the same names to their constants, so one
// translation unit cannot include both.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_dagger.h"
#include "../../include/rover_hip.h"
#include "../../include/rover_policy.h"
#include "rover_internal.hpp"
#include "offpolicy_net.hpp"
#include "train_math.hpp"

namespace {

using State = rover_dagger_state;
constexpr int NORM_BLOCKS = 64;                              // fixed chunks of the gradient's sum of squares

// ---- loss head: one thread per sampled row.  t = tanh(z) (the inference kernel's), d = t - a*, dZ6 = (d (1 - t^2)) / B; the
// row's d_0^2 + d_1^2 through the block's fixed tree to rowp[block * RP].  The label is read through the row's index, checked
// as the gather checks it (its bad_index word is already set there).
struct Head {
    const float *z;                    // the last layer's output, pitch 4
    const float *labels;               // (valid, 2)
    const int64_t *idx; int64_t valid;
    float inv_n;
    float *dz;                         // dZ6, pitch 4
    float *dz_out;                     // (rows, 2) or NULL
    int rows;
    float *rowp;
};
__global__ __launch_bounds__(FT) void dagger_head_kernel(Head A)
{
    __shared__ float red[FT];
    const int r = blockIdx.x * FT + threadIdx.x;
    float v = 0.0f;
    if (r < A.rows) {
        int64_t i = A.idx[r];
        if (i < 0 || i >= A.valid) i = 0;
        const size_t o = (size_t)r * MW[NL - 1];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float t = rv_tanhf(A.z[o + c]);
            const float d = t - A.labels[2 * i + c];
            const float tt = t * t;
            const float g = d * (1.0f - tt);
            const float dz = g * A.inv_n;
            A.dz[o + c] = dz;
            if (A.dz_out) A.dz_out[2 * (size_t)r + c] = dz;
            v = v + d * d;
        }
    }
    const float tot = block_sum(v, red);
    if (threadIdx.x == 0) A.rowp[(size_t)blockIdx.x * RP] = tot;
}

// ---- the gradient's sum of squares: workgroup b's fixed chunk to normp[b * RP]
__global__ __launch_bounds__(FT) void dagger_norm_kernel(const float *grad, int P, float *normp)
{
    __shared__ float red[FT];
    const float tot = block_sum(sumsq_partial(grad, P, NORM_BLOCKS, FT), red);
    if (threadIdx.x == 0) normp[(size_t)blockIdx.x * RP] = tot;
}

// ---- final reduce (one workgroup): the loss, the norm, clip_grad_norm_'s coefficient, the step count and Adam's scalars
__global__ __launch_bounds__(FT) void dagger_final_kernel(const float *rowp, int nblk, const float *normp, float inv_n, float max_norm,
                                                          float beta1, float beta2, float lr, rover_dagger_state *st)
{
    __shared__ float red[FT];
    float tot[1], sq[1];
    reduce_rows(rowp, nblk, 1, tot, red);
    reduce_rows(normp, NORM_BLOCKS, 1, sq, red);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(sq[0]);
        st->loss = (tot[0] * inv_n) * 0.5f;
        st->grad_norm = norm;
        st->clip_coef = max_norm > 0.0f ? grad_clip_coef(norm, max_norm) : 1.0f;
        st->steps += 1;
        adam_scalars(st->steps, beta1, beta2, lr, &st->step_size, &st->bc2_sqrt);
    }
}

// ---- Adam on the clipped gradient (train_shared.hpp's element), then the replicas
__global__ __launch_bounds__(FT) void dagger_adam_kernel(float *params, float *grad, float *m, float *v, const rover_dagger_state *st, int P,
                                                         float beta1, float beta2, float eps, float *rep, int n_copies)
{
    const int e = blockIdx.x * FT + threadIdx.x;
    if (e >= P) return;
    const float p = adam_element_clipped(params, grad, m, v, e, &st->clip_coef, &st->step_size, &st->bc2_sqrt, beta1, beta2, eps);
    refresh_replicas(rep, n_copies, (size_t)P, (size_t)e, p);
}

// ---- host side
size_t param_floats() { return (net_floats(false) + 63) & ~(size_t)63; }

// workspace: ro_s, ro_n (int64 per row), the loss's block partials, the norm's chunk partials, one network region (cache + scratch,
// ROW_F floats per row each), the weight-gradient chunk partials
size_t ws_floats(int rows)
{
    const size_t R = (size_t)rows;
    return 4 * al4(R) + rowp_floats(rows) + al4((size_t)RP * NORM_BLOCKS) + 2 * (size_t)ROW_F * R + (size_t)cdiv(rows, CH) * net_floats(false);
}
struct Ws {
    int64_t *ro_s, *ro_n;
    float *a, *r, *nt;                 // the gather's transition outputs: not asked for here
    float *rowp, *normp, *part;
    Region reg;
};
Ws ws_at(void *ws, int rows)
{
    Ws w = {};
    const size_t R = (size_t)rows;
    float *f = static_cast<float *>(ws);
    w.ro_s = reinterpret_cast<int64_t *>(f); f += 2 * al4(R);
    w.ro_n = reinterpret_cast<int64_t *>(f); f += 2 * al4(R);
    w.rowp = f; f += rowp_floats(rows);
    w.normp = f; f += al4((size_t)RP * NORM_BLOCKS);
    for (int s = 0; s < 2; ++s)
        for (int l = 0; l < NL; ++l) {
            (s ? w.reg.scr : w.reg.cache)[l] = f;
            f += (size_t)MW[l] * R;
        }
    w.part = f;
    return w;
}

}  // namespace

extern "C" {

int rover_dagger_default_hparams(rover_dagger_hparams *h)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "hparams is NULL");
    memset(h, 0, sizeof(*h));
    h->seed_lo = 42u; h->seed_hi = 0u;
    h->env_id_offset = 0;
    h->depth_clip = 10.0f; h->depth_scale = 0.1f;
    h->lr = 3e-4f;
    h->beta1 = 0.9f; h->beta2 = 0.999f; h->eps = 1e-8f;
    h->grad_norm_clip = 0.0f;
    return ROVER_OK;
}
size_t rover_dagger_hparams_bytes(void) { return sizeof(rover_dagger_hparams); }
size_t rover_dagger_state_bytes(void) { return sizeof(rover_dagger_state); }

size_t rover_dagger_param_floats(const rover_policy_desc *student)
{
    if (!is_net(student, false, ROVER_ACT_TANH, true)) return 0;
    return param_floats();
}
size_t rover_dagger_workspace_bytes(int32_t max_rows) { return max_rows > 0 ? sizeof(float) * ws_floats(max_rows) : 0; }

int rover_dagger_update(const rover_policy_desc *student, const rover_dagger_hparams *h, float *params, float *grad, float *adam_m,
                        float *adam_v, const float *obs_ring, int32_t slots, int32_t num_envs, const int32_t *ring_pos,
                        const float *labels, const int64_t *idx, int32_t n, int64_t valid_rows, void *ws, size_t ws_bytes,
                        void *state, float *replicas, int32_t n_copies, float *dz_out, void *stream)
{
    if (!student) return rover_internal_fail(ROVER_ERR_INVALID, "descriptor is NULL");
    if (!is_net(student, false, ROVER_ACT_TANH, true))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "the fused DAgger update runs the reference policy (rover_policy_default_desc(2, 1), "
                                                          "packed by rover_policy_pack) only");
    if (!h || !params || !grad || !adam_m || !adam_v || !obs_ring || !ring_pos || !labels || !idx || !ws || !state)
        return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (n < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n must be >= 1");
    if (slots < 2 || num_envs < 1) return rover_internal_fail(ROVER_ERR_INVALID, "the ring needs >= 2 slots and >= 1 env");
    if (valid_rows < 1 || valid_rows > (int64_t)(slots - 1) * num_envs)
        return rover_internal_fail(ROVER_ERR_INVALID, "valid_rows must be in [1, (slots - 1) * num_envs]");
    if (ws_bytes < rover_dagger_workspace_bytes(n)) return rover_internal_fail(ROVER_ERR_INVALID, "DAgger workspace too small");
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grad) |
         reinterpret_cast<uintptr_t>(adam_m) | reinterpret_cast<uintptr_t>(adam_v)) & 15)
        return rover_internal_fail(ROVER_ERR_INVALID, "workspace and parameter vectors must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(state) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "state must be 8-byte aligned");
    if (replicas && n_copies < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n_copies must be >= 1");
    if (!(h->grad_norm_clip >= 0.0f)) return rover_internal_fail(ROVER_ERR_INVALID, "grad_norm_clip must be >= 0");
    int dev;
    if (int rc = device_of(params, &dev)) return rc;
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    rover_dagger_state *st = static_cast<rover_dagger_state *>(state);
    Ws w = ws_at(ws, n);
    const int P = (int)net_floats(false);
    const Net pi = net_at(student, params, false);
    if (int rc = gather(w, idx, n, valid_rows, num_envs, slots, ring_pos, nullptr, nullptr, nullptr, st, s)) return rc;
    FwdJob job = {pi, w.ro_s, nullptr, 0, &w.reg};
    if (int rc = forward<State>(&job, 1, obs_ring, n, s)) return rc;
    const float inv_n = 1.0f / (float)n;
    Head H = {};
    H.z = w.reg.cache[NL - 1]; H.labels = labels; H.idx = idx; H.valid = valid_rows; H.inv_n = inv_n;
    H.dz = w.reg.scr[NL - 1]; H.dz_out = dz_out; H.rows = n; H.rowp = w.rowp;
    hipLaunchKernelGGL(dagger_head_kernel, dim3(cdiv(n, FT)), dim3(FT), 0, s, H);
    if (int rc = launched("dagger_head_kernel launch: %s")) return rc;
    Region *regs[1] = {&w.reg};
    for (int l = NL - 1; l >= 1; --l)
        if (int rc = back_layer<State>(&pi, regs, 1, l, n, s)) return rc;
    if (int rc = wgrad<State>(&pi, regs, w.ro_s, 1, obs_ring, n, w.part, grad, s)) return rc;
    hipLaunchKernelGGL(dagger_norm_kernel, dim3(NORM_BLOCKS), dim3(FT), 0, s, (const float *)grad, P, w.normp);
    hipLaunchKernelGGL(dagger_final_kernel, dim3(1), dim3(FT), 0, s, (const float *)w.rowp, cdiv(n, FT), (const float *)w.normp, inv_n,
                       h->grad_norm_clip, h->beta1, h->beta2, h->lr, st);
    if (int rc = launched("dagger final launch: %s")) return rc;
    hipLaunchKernelGGL(dagger_adam_kernel, dim3(cdiv(P, FT)), dim3(FT), 0, s, params, grad, adam_m, adam_v,
                       (const rover_dagger_state *)st, P, h->beta1, h->beta2, h->eps, replicas, (int)n_copies);
    return launched("dagger_adam_kernel launch: %s");
}

}  // extern "C"
