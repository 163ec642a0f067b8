/*
 * rover_lift_train.h -- C ABI of the fused PPO update of the lift task's networks (librover_hip.so).
 *
 * Replaces, for FrankaCubeLift-v0's networks only (rover_lift_policy_desc: MLP 36 -> 256 -> 128 -> 64 -> {8, 1}, ELU on the
 * hidden layers, no final activation, a shared log_std of 8 values), the torch autograd update of
 * isaac_rover_orbit_amd/lift_ppo.py (TorchLiftPPO, the restatement of skrl 1.1.0's PPO with the reference's
 * rover_envs/envs/manipulation/config/franka/agents/skrl_ppo_cfg.yaml): two RunningStandardScalers (states, values), the clipped
 * PPO loss (ratio clip 0.2, value clip 0.2 with clip_predicted_values, value-loss scale 2, entropy scale 0), the KL early stop
 * of an epoch, clip_grad_norm_(1.0) over both networks and log_std, one Adam, and the KL-adaptive learning rate.  Any other
 * descriptor pair returns ROVER_ERR_UNSUPPORTED; the rover's networks have their own entries (rover_train.h), which refuse these.
 *
 * Parameters live in ONE flat device vector: the policy network in the packed layout of rover_policy.h
 * (rover_policy_packed_floats(policy) floats, offsets as rover_policy_pack sets them), then the value network in the same
 * layout, then log_std (8 floats, raw, unclamped): rover_lift_ppo_param_floats() in all.  Gradients and both Adam moments have
 * the same layout; padding floats of the packed layout are written as exact zeros by every minibatch call.
 *
 * Scaler block (skrl RunningStandardScaler, device memory, 8-byte aligned, rover_lift_ppo_scaler_doubles(width) doubles):
 *     double mean[width], var[width], count;     initial state mean 0, var 1, count 1 (the caller writes it)
 *   train:    batch mean m_b and unbiased variance v_b per column (float64 sums, see the order below), count c_b = rows;
 *             delta = m_b - mean; tot = count + c_b;
 *             var = (var * count + v_b * c_b + delta^2 * count * c_b / tot) / tot;  mean = mean + delta * c_b / tot;  count = tot
 *   forward:  clamp((x - (float)mean) / (sqrtf((float)var) + scaler_eps), -clip, clip)          (fp32, no contraction)
 *   inverse:  sqrtf((float)var) * clamp(x, -clip, clip) + (float)mean                          (fp32, a product then a sum)
 * clamp propagates NaN, as torch.clamp does.
 *
 * Device state (rover_lift_ppo_state, caller-allocated, 8-byte aligned): initialise lr and zero every other field.  Within an
 * epoch the `stop` word implements skrl's KL early stop: the minibatch whose KL exceeds kl_early_stop records its KL and sets
 * `stop`; from then on every minibatch and apply call of the epoch does nothing (no scaler update, no record, no step), and the
 * stopping minibatch's own apply is skipped as skrl breaks before the optimiser step.  rover_lift_ppo_kl_schedule averages the
 * `recorded` KLs of the epoch, adapts lr and clears `stop` and `recorded`.  Nothing here synchronises with the host.
 *
 * Conventions as in rover_train.h: plain C, caller-owned DEVICE buffers, int return codes (ROVER_ERR_INVALID for a bad argument
 * or a workspace that is too small), every call asynchronous on `stream` and run on the device the first buffer lives on.
 *
 * Numerics and reduction order (bit-reproducible from run to run; no atomics):
 *   - training forward: per row and network exactly rover_policy_forward's generic kernel on the standardised rows -- the same
 *     v_mfma_f32_16x16x4_f32 sequence per 16 x 16 output tile (k groups ascending, the ragged k >= 36 lanes fed as zeros), the
 *     same bias add and the same ELU (rover_policy.h), so `mean_out` / `value_out` are bit-identical to it;
 *   - per-row gradients dL/dmean, dL/dvalue in closed form (torch.min ties pass half the gradient to each operand, torch.clamp
 *     passes it on the closed interval); backward dA = dZ W on the f32 MFMA (rows x 16 columns per tile, the n index as k in
 *     ascending quads), ELU' = y > 0 ? 1 : y + 1 from the stored activation y;
 *   - dW = dZ^T A on the f32 MFMA, one 256-thread workgroup per 16 x 16 tile: wave w accumulates the row quads w, w + 4, ...
 *     of each group of 16 quads in ascending order, the four wave partials combine as (p0 + p1) + (p2 + p3);
 *   - log_std gradient, KL and loss terms: per 16-row workgroup sequential sums, then thread t of one workgroup adds the
 *     partials t, t + 256, ... in order, then a halving tree over the 256 threads;
 *   - scaler statistics: per column, thread t of a 256-thread workgroup sums rows t, t + 256, ... in float64, then a halving
 *     tree (mean first, then the sum of squared deviations from it);
 *   - gradient norm: 128 fixed chunks of the vector, each summed like the previous item, then a halving tree.
 */
#ifndef ROVER_LIFT_TRAIN_H
#define ROVER_LIFT_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#include "rover_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Hyper-parameters; defaults = skrl_ppo_cfg.yaml of the lift task. */
typedef struct rover_lift_ppo_hparams {
    float gamma, lam;                 /* GAE discount and lambda (0.99, 0.95)                                              */
    float clip_ratio;                 /* PPO ratio clip (0.2)                                                              */
    float value_clip;                 /* clip_predicted_values range (0.2)                                                 */
    float value_loss_scale;           /* 2                                                                                 */
    float log_std_min, log_std_max;   /* clamp of log_std (-20, 2)                                                         */
    float max_grad_norm;              /* clip_grad_norm_ over both networks and log_std (1.0; torch adds 1e-6 to the norm) */
    float beta1, beta2, eps;          /* Adam (0.9, 0.999, 1e-8)                                                           */
    float kl_threshold;               /* KLAdaptiveRL: lr / factor above 2 x threshold, lr x factor below threshold / 2 (0.008) */
    float lr_factor;                  /* 1.5                                                                               */
    float lr_min, lr_max;             /* 1e-6, 1e-2                                                                        */
    float kl_early_stop;              /* skrl's kl_threshold: stop the epoch once a minibatch KL exceeds it (0.008; 0 = off) */
    float reward_scale;               /* rewards_shaper_scale (0.01), applied by the caller's rollout                      */
    float scaler_eps, scaler_clip;    /* RunningStandardScaler epsilon and clip_threshold (1e-8, 5)                        */
} rover_lift_ppo_hparams;

/* Device-resident optimiser state (48 bytes). */
typedef struct rover_lift_ppo_state {
    double lr;          /* learning rate; rover_lift_ppo_kl_schedule updates it on the device                             */
    int32_t step;       /* Adam steps taken                                                                               */
    float grad_norm;    /* global gradient norm of the last apply that ran, before clipping                              */
    float clip_coef;    /* min(1, max_grad_norm / (grad_norm + 1e-6)) of that apply                                       */
    float step_size;    /* (float)(lr / (1 - beta1^step)) of that apply                                                   */
    float bc2_sqrt;     /* (float)sqrt(1 - beta2^step) of that apply                                                      */
    int32_t stop;       /* nonzero: this epoch stopped early (KL above kl_early_stop)                                     */
    int32_t recorded;   /* minibatch KLs recorded in this epoch                                                           */
    int32_t epochs;     /* epochs closed by rover_lift_ppo_kl_schedule                                                    */
    int32_t stopped_epochs; /* of those, epochs that stopped early                                                        */
    int32_t reserved;
} rover_lift_ppo_state;

int rover_lift_ppo_default_hparams(rover_lift_ppo_hparams *h);
size_t rover_lift_ppo_hparams_bytes(void);
size_t rover_lift_ppo_state_bytes(void);

/* Floats of the flat parameter vector of a lift policy / value pair (policy rover_lift_policy_desc(8), value (1), packed by
 * rover_policy_pack); 0 for any other pair. */
size_t rover_lift_ppo_param_floats(const rover_policy_desc *policy, const rover_policy_desc *value);
/* Device workspace bytes for minibatches of up to `max_rows` rows (also enough for apply and standardize); 0 if max_rows <= 0. */
size_t rover_lift_ppo_workspace_bytes(int32_t max_rows);
/* Doubles of a scaler block of `width` columns (2 width + 1); 0 if width < 1 or width > 64. */
size_t rover_lift_ppo_scaler_doubles(int32_t width);

/* out = scaler(x) with h's scaler_eps / scaler_clip (train: update the statistics with all `rows` rows first, then standardise with the new ones; inverse: the
 * inverse transform, no update).  x / out (rows, width) fp32, may alias; scaler: the block above.  ws: at least
 * rover_lift_ppo_workspace_bytes(1) bytes, used by train only (may be NULL otherwise).  rows >= 2 for train. */
int rover_lift_ppo_standardize(const rover_lift_ppo_hparams *h, double *scaler, int32_t width, const float *x, int32_t rows,
                               int32_t train, int32_t inverse, float *out, void *ws, size_t ws_bytes, void *stream);

/* One minibatch of rows idx[0 .. n) of the flat rollout buffers (B rows): obs (B, 36) RAW observations, act (B, 8),
 * logp / val / ret / adv (B) -- val and ret already standardised by the value scaler.  Unless `state->stop` is set:
 *   1. if train_scaler (the first epoch): update state_scaler (width 36) with the n gathered raw rows;
 *   2. standardise the rows with state_scaler, forward both networks, the loss and its gradient into `grad` (overwritten);
 *   3. stats (4 floats): mean KL ((r - 1) - log r), policy loss, value loss (scaled), 0; state->recorded += 1; state->stop = 1
 *      if the KL exceeds h->kl_early_stop (> 0).
 * mean_out (n, 8) / value_out (n, 1) receive the forward's outputs when not NULL.  idx: int64, any order, repeats allowed. */
int rover_lift_ppo_minibatch(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_lift_ppo_hparams *h,
                             const float *params, double *state_scaler, const float *obs, const float *act, const float *logp,
                             const float *val, const float *ret, const float *adv, const int64_t *idx, int32_t n,
                             int32_t train_scaler, void *state, void *ws, size_t ws_bytes, float *grad, float *stats,
                             float *mean_out, float *value_out, void *stream);

/* Unless state->stop is set: clip_grad_norm_ + one Adam step in torch's order (as rover_ppo_apply), then the new packed
 * parameters of each network n_copies times back to back into replicas_policy / replicas_value (either may be NULL).  `grad` is
 * overwritten: after a step that ran it holds the clipped gradient, grad * state->clip_coef (fp32 products). */
int rover_lift_ppo_apply(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_lift_ppo_hparams *h,
                         float *params, float *grad, float *adam_m, float *adam_v, void *state, float *replicas_policy,
                         float *replicas_value, int32_t n_copies, void *ws, size_t ws_bytes, void *stream);

/* End of an epoch, one thread on the device: kl = (sum of stats[4 m], m = 0 .. state->recorded, in order) / recorded (the
 * first `recorded` of the n_minibatches records, the stopping one included); lr = max(lr / factor, lr_min) if
 * kl > 2 threshold, min(lr x factor, lr_max) if kl < threshold / 2 (double); then stop = recorded = 0.  kl_out (1 float, may be
 * NULL) receives kl. */
int rover_lift_ppo_kl_schedule(const rover_lift_ppo_hparams *h, const float *stats, int32_t n_minibatches, void *state,
                               float *kl_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_LIFT_TRAIN_H */
