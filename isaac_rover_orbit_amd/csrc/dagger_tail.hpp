// dagger_tail.hpp -- what the two fused DAgger updates share (dagger_kernels.hip, dagger_conv_kernels.hip): the imitation loss head
// with its closed-form tanh backward, the gradient's norm, the final reduce into the device state and Adam with
// clip_grad_norm_'s coefficient (rover_dagger.h), the refusals of the update entry points, the common part of the workspace and
// the launchers of the head and of the tail.
//
// Include it after offpolicy_net.hpp and train_math.hpp.  Everything is in an unnamed namespace, as in offpolicy_net.hpp: each
// translation unit gets its own internal-linkage copy of the four kernels and nothing needs -fgpu-rdc.
#ifndef ROVER_DAGGER_TAIL_HPP
#define ROVER_DAGGER_TAIL_HPP

#include "../../include/rover_dagger.h"
#include "collect_record.hpp"

namespace {

using State = rover_dagger_state;                            // offpolicy_net.hpp's templates run under this trainer's state
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

// ---- Adam on the clipped gradient (train_shared.hpp's element) over all P floats, then the replicas of the first `head`
__global__ __launch_bounds__(FT) void dagger_adam_kernel(float *params, float *grad, float *m, float *v, const rover_dagger_state *st, int P,
                                                         int head, float beta1, float beta2, float eps, float *rep, int n_copies)
{
    const int e = blockIdx.x * FT + threadIdx.x;
    if (e >= P) return;
    const float p = adam_element_clipped(params, grad, m, v, e, &st->clip_coef, &st->step_size, &st->bc2_sqrt, beta1, beta2, eps);
    if (e < head) refresh_replicas(rep, n_copies, (size_t)head, (size_t)e, p);
}

// ---- host side
size_t head_floats() { return (net_floats(false) + 63) & ~(size_t)63; }          // rover_dagger_param_floats

// What rover_dagger_update and rover_dagger_conv_update refuse, in the order and with the texts of both.  `im` is the conv
// trainer's (NULL otherwise): its three refusals stand where its caller has always met them, between the shared ones, so a call
// that breaks two rules gets the message it got; its image ring also joins the alignment rule, under that rule's conv text.
struct UpdateImage {
    bool size_ok;
    const float *ring;
    int32_t slots;
};
int update_check(const rover_policy_desc *student, const rover_dagger_hparams *h, const float *params, const float *grad,
                 const float *adam_m, const float *adam_v, const float *obs_ring, int32_t slots, int32_t num_envs,
                 const int32_t *ring_pos, const float *labels, const int64_t *idx, int32_t n, int64_t valid_rows, const void *ws,
                 size_t ws_bytes, size_t ws_need, const void *state, const float *replicas, int32_t n_copies, const UpdateImage *im)
{
    if (!student) return rover_internal_fail(ROVER_ERR_INVALID, "descriptor is NULL");
    if (!is_net(student, false, ROVER_ACT_TANH, true))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "the fused DAgger update runs the reference policy (rover_policy_default_desc(2, 1), "
                                                          "packed by rover_policy_pack) only");
    if (im && !im->size_ok) return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "the stem reads 90 x 160 images only");
    if (!h || !params || !grad || !adam_m || !adam_v || !obs_ring || (im && !im->ring) || !ring_pos || !labels || !idx || !ws || !state)
        return rover_internal_fail(ROVER_ERR_INVALID, "NULL argument");
    if (n < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n must be >= 1");
    if (slots < 2 || num_envs < 1) return rover_internal_fail(ROVER_ERR_INVALID, "the ring needs >= 2 slots and >= 1 env");
    if (im && im->slots < slots)
        return rover_internal_fail(ROVER_ERR_INVALID, "the image ring must have the observation ring's slots or more");
    if (valid_rows < 1 || valid_rows > (int64_t)(slots - 1) * num_envs)
        return rover_internal_fail(ROVER_ERR_INVALID, "valid_rows must be in [1, (slots - 1) * num_envs]");
    if (ws_bytes < ws_need) return rover_internal_fail(ROVER_ERR_INVALID, "DAgger workspace too small");
    if (misaligned(ws) || misaligned(params) || misaligned(grad) || misaligned(adam_m) || misaligned(adam_v) || (im && misaligned(im->ring)))
        return rover_internal_fail(ROVER_ERR_INVALID, im ? "workspace, parameter vectors and image ring must be 16-byte aligned"
                                                         : "workspace and parameter vectors must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(state) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "state must be 8-byte aligned");
    if (replicas && n_copies < 1) return rover_internal_fail(ROVER_ERR_INVALID, "n_copies must be >= 1");
    if (!(h->grad_norm_clip >= 0.0f)) return rover_internal_fail(ROVER_ERR_INVALID, "grad_norm_clip must be >= 0");
    return ROVER_OK;
}

// The workspace both updates share: ro_s, ro_n (int64 per row) | gap0 | the loss's block partials, the norm's chunk partials |
// gap1 | one network region (cache + scratch, ROW_F floats per row each), the weight-gradient chunk partials | what the caller
// appends.  The gaps are the conv trainer's (ident; the gathered rows and dRow) and 0 floats wide otherwise.
struct Ws {
    int64_t *ro_s, *ro_n;
    float *a, *r, *nt;                 // the gather's transition outputs: not asked for here
    float *rowp, *normp, *part;
    Region reg;
};
size_t ws_shared_floats(int rows)
{
    const size_t R = (size_t)rows;
    return 4 * al4(R) + rowp_floats(rows) + al4((size_t)RP * NORM_BLOCKS) + 2 * (size_t)ROW_F * R + (size_t)cdiv(rows, CH) * net_floats(false);
}
// fills w; at0 / at1 receive where the gaps start; returns the first float behind `part`
float *ws_carve(Ws &w, void *ws, int rows, size_t gap0 = 0, float **at0 = nullptr, size_t gap1 = 0, float **at1 = nullptr)
{
    const size_t R = (size_t)rows;
    float *f = static_cast<float *>(ws);
    w.ro_s = reinterpret_cast<int64_t *>(f); f += 2 * al4(R);
    w.ro_n = reinterpret_cast<int64_t *>(f); f += 2 * al4(R);
    if (at0) *at0 = f;
    f += gap0;
    w.rowp = f; f += rowp_floats(rows);
    w.normp = f; f += al4((size_t)RP * NORM_BLOCKS);
    if (at1) *at1 = f;
    f += gap1;
    for (int s = 0; s < 2; ++s)
        for (int l = 0; l < NL; ++l) {
            (s ? w.reg.scr : w.reg.cache)[l] = f;
            f += (size_t)MW[l] * R;
        }
    w.part = f;
    return f + (size_t)cdiv(rows, CH) * net_floats(false);
}

// the loss head over the region's last layer: dZ6 into its scratch, the block partials into rowp
int dagger_head(const Ws &w, const float *labels, const int64_t *idx, int64_t valid_rows, int n, float *dz_out, hipStream_t s)
{
    Head H = {};
    H.z = w.reg.cache[NL - 1]; H.labels = labels; H.idx = idx; H.valid = valid_rows; H.inv_n = 1.0f / (float)n;
    H.dz = w.reg.scr[NL - 1]; H.dz_out = dz_out; H.rows = n; H.rowp = w.rowp;
    hipLaunchKernelGGL(dagger_head_kernel, dim3(cdiv(n, FT)), dim3(FT), 0, s, H);
    return launched("dagger_head_kernel launch: %s");
}

// norm, final and Adam over the P floats of `grad`; the replicas hold the first `head` floats of params
int dagger_tail(const rover_dagger_hparams *h, float *params, float *grad, float *adam_m, float *adam_v, int P, int head, const Ws &w,
                int n, rover_dagger_state *st, float *replicas, int n_copies, hipStream_t s)
{
    hipLaunchKernelGGL(dagger_norm_kernel, dim3(NORM_BLOCKS), dim3(FT), 0, s, (const float *)grad, P, w.normp);
    hipLaunchKernelGGL(dagger_final_kernel, dim3(1), dim3(FT), 0, s, (const float *)w.rowp, cdiv(n, FT), (const float *)w.normp,
                       1.0f / (float)n, h->grad_norm_clip, h->beta1, h->beta2, h->lr, st);
    if (int rc = launched("dagger final launch: %s")) return rc;
    hipLaunchKernelGGL(dagger_adam_kernel, dim3(cdiv(P, FT)), dim3(FT), 0, s, params, grad, adam_m, adam_v, (const rover_dagger_state *)st,
                       P, head, h->beta1, h->beta2, h->eps, replicas, n_copies);
    return launched("dagger_adam_kernel launch: %s");
}

}  // namespace

#endif  // ROVER_DAGGER_TAIL_HPP
