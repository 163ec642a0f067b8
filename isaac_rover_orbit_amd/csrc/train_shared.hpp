// train_shared.hpp -- what the trainers' translation units share beyond the scalar math of train_math.hpp (gfx950 / CDNA4, wave64):
// the packed-layout helpers (device and host) and the optimiser tail (the gradient's sum of squares, clip_grad_norm_'s
// coefficient, Adam's bias-correction scalars, the Adam element, the replica refresh, the KL-adaptive rate rule).  Read by
// ppo_kernels.hip, lift_ppo_kernels.hip, trpo_kernels.hip, offpolicy_net.hpp (TD3, SAC) and lift_rollout_kernels.hip (layout only).
//
// Shared are device functions, not kernels: every __global__ stays in its own file under its own name.  Everything here is
// force-inlined and was shaped until each kernel compiled to what it was with the text in place (profiles/onpolicy_share_isa.txt,
// tools/isa_same.py).  That rule decided three things:
//   - there is no one "prep" function from the summed squares to the four scalars: the kernels store the norm and the coefficient
//     before the two pow() calls, and a function that returns all four moves that store and with it the schedule.
//     grad_clip_coef and adam_scalars are its halves, the second is also all the off-policy trainers need;
//   - the two-block replica refresh of the PPO updates (policy replicas, value replicas, none for log_std) and ppo_kl_kernel's rate
//     rule stay written out in their kernels: behind a call their branches come out in another order;
//   - ppo_wgrad_kernel and lift_wgrad_kernel keep their text.  A device function that is handed the kernel's argument struct moves
//     the kernel (the struct's copy is then taken apart later in the pipeline), and one that is handed the decoded job as scalars
//     moves lift's kernel too.
//
// block_sum is not here on purpose.  The three forms (ppo_kernels.hip: no trailing barrier, the total in thread 0;
// lift_ppo_kernels.hip: a trailing barrier, every thread; trpo_kernels.hip / offpolicy_net.hpp: a leading barrier, every thread)
// place their barriers where their callers need them; one form would move the instruction stream of some twenty kernels and save
// ten lines.  TRPO's dense / JVP / backward and chunked weight-gradient kernels resemble offpolicy_net.hpp's and are not shared
// with it either: they carry the JVP operands and the skip word, and folding them is a change of its own.
//
// policy_kernels.hip keeps its own layer_weight_floats / layer_bias_floats: that file's text does not move, which is
// also why the packed sizes are here and not in rover_internal.hpp, which it includes.
#ifndef ROVER_TRAIN_SHARED_HPP
#define ROVER_TRAIN_SHARED_HPP

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/rover_policy.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));   // an MFMA accumulator, a packed weight fragment

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ inline size_t al4(size_t n) { return (n + 3) & ~(size_t)3; }

// W[n][k] of a packed layer with G k groups (rover_policy.h "Packed weights"): fragment (t = n / 16, g = k / 16), lane
// (n & 15) + 16 (k & 3), element (k & 15) / 4
__device__ __forceinline__ float w_at(const float *Wp, int G, int n, int k)
{
    return Wp[((((size_t)(n >> 4) * G + (k >> 4)) * 64 + (n & 15) + 16 * (k & 3)) << 2) + ((k >> 2) & 3)];
}

// ---- packed sizes (host): floats of a layer's weight fragments and of its padded bias, and of a whole descriptor
inline size_t layer_weight_floats(int N, int K) { return (size_t)cdiv(N, 16) * cdiv(K, 16) * 64 * 4; }
inline size_t layer_bias_floats(int N) { return al4((size_t)N); }
inline size_t layer_weight_floats(const rover_policy_layer &l) { return layer_weight_floats(l.N, l.K); }
inline size_t layer_bias_floats(const rover_policy_layer &l) { return layer_bias_floats(l.N); }
inline size_t packed_floats(const rover_policy_desc *d)
{
    size_t n = 0;
    for (int i = 0; i < d->n_enc + d->n_mlp; ++i) n += layer_weight_floats(d->layers[i]) + layer_bias_floats(d->layers[i]);
    return n;
}
// the reference architecture (rover_policy_default_desc), final tanh iff out_dim 2 (policy) / none iff 1 (value), with the
// offsets rover_policy_pack sets
inline bool is_reference(const rover_policy_desc *d, int nout, int final_act)
{
    constexpr int NL = 6, K[NL] = {961, 80, 64, 256, 160, 128}, N[NL - 1] = {80, 60, 256, 160, 128};
    if (!d) return false;
    if (d->obs_dim != 965 || d->prop_dim != 4 || d->enc_offset != 3 || d->enc_dim != K[0] || d->n_enc != 2 || d->n_mlp != 4)
        return false;
    if (d->leaky_slope != 0.01f) return false;
    size_t off = 0;
    for (int i = 0; i < NL; ++i) {
        const rover_policy_layer &l = d->layers[i];
        if (l.K != K[i] || l.N != (i < NL - 1 ? N[i] : nout)) return false;
        if (l.act != (i < NL - 1 ? ROVER_ACT_LEAKY_RELU : final_act)) return false;
        if ((l.split_k != 0) != (i == 0 || i == NL - 1)) return false;
        if (l.w_off != off) return false;
        off += layer_weight_floats(l);
        if (l.b_off != off) return false;
        off += layer_bias_floats(l);
    }
    return true;
}

// ---- clip_grad_norm_ + Adam
// this thread's share of workgroup blockIdx.x's chunk of sum grad^2 (nblocks fixed chunks, threads strided); the caller reduces
__device__ __forceinline__ float sumsq_partial(const float *grad, int P, int nblocks, int threads)
{
    const int chunk = cdiv(P, nblocks), e0 = blockIdx.x * chunk, e1 = min(e0 + chunk, P);
    float s = 0.0f;
    for (int e = e0 + threadIdx.x; e < e1; e += threads) s += grad[e] * grad[e];
    return s;
}

// clip_grad_norm_'s coefficient for a gradient of norm `norm`
__device__ __forceinline__ float grad_clip_coef(float norm, float max_norm)
{
    const float coef = max_norm / (norm + 1e-6f);
    return fminf(coef, 1.0f);
}
// torch's bias corrections of step `step` in double: lr / bc1 as step_size, sqrt(bc2).  lr as the caller holds it (the state's
// double, a float hyper-parameter): it is widened where it is used, behind the pow() calls
template <class LR>
__device__ __forceinline__ void adam_scalars(int step, float beta1, float beta2, LR lr, float *step_size, float *bc2_sqrt)
{
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    *step_size = (float)((double)lr / bc1);
    *bc2_sqrt = (float)sqrt(bc2);
}
// Adam (torch's single-tensor order) on element e with gradient g; returns the new parameter.  The two scalars are read through
// their pointers where torch's order uses them: behind the caller's stores, which the compiler cannot tell apart from them.
__device__ __forceinline__ float adam_element(float *params, float *m, float *v, int e, float g, const float *step_size,
                                              const float *bc2_sqrt, float beta1, float beta2, float eps)
{
    const float w1 = (float)(1.0 - (double)beta1), w2 = (float)(1.0 - (double)beta2);
    const float mo = m[e], mn = mo + w1 * (g - mo);                     // exp_avg.lerp_(grad, 1 - beta1)
    const float vn = v[e] * beta2 + w2 * (g * g);                       // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    const float denom = sqrtf(vn) / *bc2_sqrt + eps;                    // (exp_avg_sq.sqrt() / sqrt(bc2)).add_(eps)
    const float p = params[e] + (-*step_size) * (mn / denom);           // param.addcdiv_(exp_avg, denom, -lr / bc1)
    m[e] = mn;
    v[e] = vn;
    params[e] = p;
    return p;
}
// the on-policy form: the gradient times clip_grad_norm_'s coefficient first, written back (the trainers report it)
__device__ __forceinline__ float adam_element_clipped(float *params, float *grad, float *m, float *v, int e, const float *clip_coef,
                                                      const float *step_size, const float *bc2_sqrt, float beta1, float beta2,
                                                      float eps)
{
    const float g = grad[e] * *clip_coef;
    grad[e] = g;
    return adam_element(params, m, v, e, g, step_size, bc2_sqrt, beta1, beta2, eps);
}

// the new parameter into element e of every replica of a P-float block (rep NULL: there are none)
__device__ __forceinline__ void refresh_replicas(float *rep, int n_copies, size_t P, size_t e, float p)
{
    if (rep)
        for (int c = 0; c < n_copies; ++c) rep[c * P + e] = p;
}

// skrl's KLAdaptiveLR in double: lr / factor above 2 thr, lr * factor below thr / 2
__device__ __forceinline__ double kl_adaptive_lr(double lr, float kl, float thr, float factor, float lr_min, float lr_max)
{
    if ((double)kl > 2.0 * (double)thr) lr = fmax(lr / (double)factor, (double)lr_min);
    else if ((double)kl < 0.5 * (double)thr) lr = fmin(lr * (double)factor, (double)lr_max);
    return lr;
}

}  // namespace

#endif  // ROVER_TRAIN_SHARED_HPP
