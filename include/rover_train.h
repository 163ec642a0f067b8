/*
 * rover_train.h -- C ABI of the fused PPO update of the rover networks (librover_hip.so).
 *
 * Replaces, for the reference architecture only (rover_policy_default_desc: encoder 961 -> 80 -> 60 on obs[:, 3:-1], MLP
 * (4 + 60) -> 256 -> 160 -> 128 -> {2 + tanh, 1}, LeakyReLU 0.01, a shared log_std of 2 values), the torch autograd update of
 * examples/04_train_ppo.py: its GAE loop, the clipped PPO loss (ratio clip, value clip with clip_predicted_values, value-loss
 * scale 1, entropy scale 0), clip_grad_norm_ over both networks, one Adam over both networks and the KL-adaptive learning rate.
 * Any other descriptor returns ROVER_ERR_UNSUPPORTED.
 *
 * Parameters live in ONE flat device vector: the policy network in the packed layout of rover_policy.h ("Packed weights",
 * rover_policy_packed_floats(policy) floats, offsets as rover_policy_pack sets them), then the value network in the same
 * layout, then log_std (2 floats, raw, unclamped) and 2 floats of padding: rover_ppo_param_floats() in all.  Gradients and
 * the two Adam moments have the same layout.  Padding floats of the packed layout are written as exact zeros by every
 * minibatch call, so their Adam moments and parameters stay exactly zero.
 *
 * Conventions as in rover_hip.h: plain C, caller-owned DEVICE buffers, int return codes (ROVER_ERR_INVALID for a bad
 * argument, n <= 0 or a workspace that is too small), rover_last_error() for the text, every call asynchronous on `stream`
 * and run on the device the parameter vector lives on.  Nothing here synchronises with the host.
 *
 * Numerics and reduction order (every result is bit-reproducible from run to run whatever the launch order; no atomics):
 *   - training forward: per row and per network exactly rover_policy_forward_pair's arithmetic (same k-ordered fmaf chains,
 *     same split-K cuts and combine order, same rv_tanhf), so `mean` / `value` are bit-identical to RoverNet on the same rows;
 *   - per-row gradients dL/dmean, dL/dvalue in closed form (torch's conventions: min / clamp ties pass half / all of the
 *     gradient as torch.min and torch.clamp do); backward dA = dZ W row-parallel in fp32, LeakyReLU' from the sign of the
 *     stored activation, tanh' = 1 - y^2;
 *   - weight / bias gradients dW = sum_rows dZ^T A on the f32 MFMA, one 256-thread workgroup per 16 x 16 tile: wave w
 *     accumulates the row quads w, w + 4, w + 8, ... in ascending order, the four partials combine as (p0 + p1) + (p2 + p3);
 *   - log_std gradient, KL and the loss terms: per 16-row workgroup sequential sums over its rows, then one workgroup adds
 *     the workgroup partials -- thread t sums partials t, t + 256, ... in order, then a fixed halving tree over the threads;
 *   - gradient norm: 128 fixed chunks of the gradient vector, each summed like the previous item, then a halving tree.
 */
#ifndef ROVER_TRAIN_H
#define ROVER_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#include "rover_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Hyper-parameters; defaults = examples/04_train_ppo.py (the reference's rover_ppo.yaml). */
typedef struct rover_ppo_hparams {
    float gamma, lam;                 /* GAE discount and lambda (0.99, 0.95)                                            */
    float clip_ratio;                 /* PPO ratio clip (0.2)                                                            */
    float value_clip;                 /* clip_predicted_values range (0.2)                                               */
    float value_loss_scale;           /* 1                                                                               */
    float log_std_min, log_std_max;   /* clamp of log_std (-20, 2)                                                       */
    float max_grad_norm;              /* clip_grad_norm_ over both networks (0.5; torch adds 1e-6 to the norm)           */
    float beta1, beta2, eps;          /* Adam (0.9, 0.999, 1e-8)                                                         */
    float kl_threshold;               /* KL-adaptive rate: lr / factor above 2 x threshold, lr x factor below threshold / 2 (0.008) */
    float lr_factor;                  /* 1.5                                                                             */
    float lr_min, lr_max;             /* 1e-6, 1e-2                                                                      */
} rover_ppo_hparams;

/* Device-resident optimiser state (caller-allocated, 32 bytes, 8-byte aligned).  Initialise lr and step = 0 before the
 * first rover_ppo_apply; the other fields are written by the library. */
typedef struct rover_ppo_state {
    double lr;          /* learning rate; rover_ppo_kl_schedule updates it on the device                                    */
    int32_t step;       /* Adam steps taken                                                                                 */
    float grad_norm;    /* global gradient norm of the last rover_ppo_apply, before clipping                                */
    float clip_coef;    /* min(1, max_grad_norm / (grad_norm + 1e-6)) of the last apply                                     */
    float step_size;    /* (float)(lr / (1 - beta1^step)) of the last apply                                                 */
    float bc2_sqrt;     /* (float)sqrt(1 - beta2^step) of the last apply                                                    */
    float reserved;
} rover_ppo_state;

int rover_ppo_default_hparams(rover_ppo_hparams *h);
/* sizeof(rover_ppo_hparams) / sizeof(rover_ppo_state): let a binding check its mirrors of the structs. */
size_t rover_ppo_hparams_bytes(void);
size_t rover_ppo_state_bytes(void);

/* Floats of the flat parameter vector for this policy / value pair (see above); 0 if a descriptor is invalid. */
size_t rover_ppo_param_floats(const rover_policy_desc *policy, const rover_policy_desc *value);
/* Device workspace bytes for minibatches of up to `max_rows` rows (also enough for rover_ppo_apply); 0 if max_rows <= 0. */
size_t rover_ppo_workspace_bytes(int32_t max_rows);

/* One minibatch: forward of both networks on rows idx[0 .. n) of the flat rollout buffers, the PPO loss and its gradient
 * with respect to every parameter into `grad` (fully overwritten).  Rollout buffers (B = T x num_envs rows, row-major):
 * obs (B, 965), act (B, 2), logp / val / ret / adv (B).  idx: int64 row indices (torch.randperm), any order, repeats allowed.
 * stats: 4 floats -- mean KL ((r - 1) - log r), policy loss, value loss (scaled), 0.  mean_out (n, 2) / value_out (n, 1)
 * receive the forward's outputs when not NULL.  ws: rover_ppo_workspace_bytes(n) bytes or more, 16-byte aligned. */
int rover_ppo_minibatch(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_ppo_hparams *h,
                        const float *params, const float *obs, const float *act, const float *logp, const float *val,
                        const float *ret, const float *adv, const int64_t *idx, int32_t n, void *ws, size_t ws_bytes,
                        float *grad, float *stats, float *mean_out, float *value_out, void *stream);

/* clip_grad_norm_ + one Adam step (torch's order of operations: step size lr / bc1, denominator sqrt(v) / sqrt(bc2) + eps) of
 * `params` with `grad`, moments `adam_m` / `adam_v`; `state` (rover_ppo_state, device) supplies lr and counts the step.
 * Then writes the new packed parameters of each network `n_copies` times back to back into replicas_policy /
 * replicas_value -- the buffers rover_policy_forward / rover_policy_forward_pair read with that n_copies (either may be
 * NULL).  ws: >= rover_ppo_workspace_bytes(1) bytes.  `grad` is left scaled by the clip coefficient, as torch leaves it. */
int rover_ppo_apply(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_ppo_hparams *h, float *params,
                    float *grad, float *adam_m, float *adam_v, void *state, float *replicas_policy, float *replicas_value,
                    int32_t n_copies, void *ws, size_t ws_bytes, void *stream);

/* Generalised advantage estimation, one thread per env, reverse over t in examples/04_train_ppo.py's exact fp32 order:
 *   nv = t == T - 1 ? last_v : val[t + 1];  nd = 1 - done[t];
 *   delta = (rew[t] + (gamma * nv) * nd) - val[t];  gae = delta + ((gamma * lam) * nd) * gae;  adv[t] = gae;  ret[t] = adv[t] + val[t]
 * with gamma and gamma * lam rounded to fp32 (gamma * lam formed in double, as Python does).  rew / done / val / adv / ret
 * (T, n_envs), last_v (n_envs).  The advantage normalisation is left to the caller. */
int rover_ppo_gae(const rover_ppo_hparams *h, const float *rew, const float *done, const float *val, const float *last_v,
                  int32_t T, int32_t n_envs, float *adv, float *ret, void *stream);

/* KL-adaptive learning rate after an epoch, one thread on the device: kl = (sum of stats[4 m], m = 0 .. n_minibatches, in
 * order) / n_minibatches; lr = max(lr / factor, lr_min) if kl > 2 threshold, min(lr x factor, lr_max) if kl < threshold / 2
 * (double, as the example's Python floats).  `stats` = the n_minibatches consecutive 4-float records rover_ppo_minibatch
 * wrote; kl_out (1 float, may be NULL) receives kl. */
int rover_ppo_kl_schedule(const rover_ppo_hparams *h, const float *stats, int32_t n_minibatches, void *state, float *kl_out,
                          void *stream);

/* Host only (pure CPU): the inverse of rover_policy_pack -- weights[i] (N, K) row-major and biases[i] (N) of every layer from a
 * packed buffer (host memory) laid out by rover_policy_pack with this descriptor. */
int rover_policy_unpack(const rover_policy_desc *d, const float *packed, float *const *weights, float *const *biases);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_TRAIN_H */
