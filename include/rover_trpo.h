/*
 * rover_trpo.h -- C ABI of the fused TRPO update of the rover networks (librover_hip.so).
 *
 * skrl 1.x TRPO._update with the reference's rover_trpo.yaml and get_model_gaussian models, for the reference architecture
 * only (the same policy / value pair as rover_train.h; any other descriptor returns ROVER_ERR_UNSUPPORTED):
 *   1. surrogate L = mean_r adv_r exp(lp_r(theta) - logp_r) over all B rows and its gradient g at theta_old;
 *   2. Fisher-vector products F v = (1/B) sum_r J_r^T diag(sigma^-2) J_r v_w (network block, J_r = dmean_r / dw), 2 c_i v_s,i
 *      (log_std block, c_i = 1 inside the clamp of log_std, else 0), plus damping v -- the double-backward of the mean
 *      KL(theta_old || theta) at theta = theta_old, where only the Gauss-Newton term survives;
 *   3. conjugate gradient on F x = g, skrl's loop and residual rule;
 *   4. step = sqrt(2 max_kl / x.F x), full = step x, expected improvement E = g.full;
 *   5. backtracking alpha_i = step_fraction 0.5^i, E *= alpha_i (skrl's cumulative product), accept the first trial with
 *      KL < max_kl and (L - L_old) / E > accept_ratio; with none accepted theta_old is restored bit for bit;
 *   6. value regression: value_loss_scale mse(ret, V(obs)) per minibatch, clip_grad_norm_ over the value network, Adam.
 *
 * Parameters live in ONE flat device vector laid out as rover_train.h's: policy packed, value packed, log_std (2 raw floats)
 * and 2 floats of padding; rover_trpo_param_floats() floats in all (the same number as rover_ppo_param_floats).  The
 * policy-side vectors of this header (g, v, F v) have the same length and layout: their value block is written as zeros.
 * Padding floats of the packed layout are written as zeros; a direction v must hold zeros there.
 *
 * Conventions as in rover_train.h: plain C, caller-owned DEVICE buffers, int return codes, every call asynchronous on
 * `stream`, no host synchronisation, no atomics.  The state struct lives in device memory: its cg_done / ls_done words work
 * like the lift trainer's stop word -- every later kernel of the launch sequence reads them first and returns at once.
 *
 * Numerics and reduction order (bit-reproducible from run to run; results are fp32 and agree with float64, not bit for bit
 * with torch):
 *   - dense layers (forward, forward-mode JVP dZ = W dA + dW A + db, reverse dA = dZ W) on v_mfma_f32_16x16x4_f32, the
 *     reduction over k in ascending groups of 4 (one MFMA per group); LeakyReLU' from the sign of the stored activation,
 *     tanh' = 1 - y^2;
 *   - weight / bias gradients dW = sum_rows dZ^T A: rows cut into fixed chunks of 2048, one MFMA chain per (tile, chunk) over
 *     the chunk's rows in ascending groups of 4, then the chunk partials added in chunk order;
 *   - per-row terms (surrogate, log_std gradient, KL, value loss): per 256-row block a fixed halving tree, then one workgroup:
 *     thread t adds block partials t, t + 256, ... in order, then a fixed halving tree;
 *   - dot products and norms: 128 fixed chunks of the vector, each summed like the previous item, then a halving tree.
 */
#ifndef ROVER_TRPO_H
#define ROVER_TRPO_H

#include <stddef.h>
#include <stdint.h>

#include "rover_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Hyper-parameters; defaults = skrl TRPO_DEFAULT_CONFIG with rover_trpo.yaml (the yaml's learning_rate 1e-4 is not a TRPO
 * key: skrl's TRPO reads value_learning_rate). */
typedef struct rover_trpo_hparams {
    float gamma, lam;                 /* GAE (0.99, 0.95), as rover_ppo_gae reads them                                    */
    float value_loss_scale;           /* 1                                                                                */
    float log_std_min, log_std_max;   /* clamp of log_std (-20, 2)                                                        */
    float max_grad_norm;              /* clip_grad_norm_ over the value network (0.5; torch adds 1e-6 to the norm)        */
    float beta1, beta2, eps;          /* value Adam (0.9, 0.999, 1e-8)                                                    */
    float value_lr;                   /* value_learning_rate (1e-3)                                                       */
    float damping;                    /* 0.1                                                                              */
    float max_kl;                     /* max_kl_divergence (0.01)                                                         */
    float cg_tol;                     /* CG residual tolerance on r.r (1e-10)                                             */
    float accept_ratio;               /* 0.5                                                                              */
    float step_fraction;              /* 1                                                                                */
    int32_t cg_steps;                 /* conjugate_gradient_steps (10)                                                    */
    int32_t max_backtrack;            /* max_backtrack_steps (10)                                                         */
} rover_trpo_hparams;

/* Device-resident state (caller-allocated, 96 bytes, 8-byte aligned, zero it once before the first call).  The policy
 * entries (rover_trpo_policy_grad starts each update) reset every field but value_step; the library writes all fields. */
typedef struct rover_trpo_state {
    int32_t cg_done;        /* 1 once r.r < cg_tol: later CG kernels return at once                                       */
    int32_t ls_done;        /* 1 once a line-search trial is accepted: later trial kernels return at once                 */
    int32_t accepted;       /* accepted trial index; -1 while searching and after a restore                               */
    int32_t cg_iters;       /* CG iterations run                                                                           */
    int32_t trials;         /* line-search trials run                                                                      */
    int32_t value_step;     /* value Adam steps taken (never reset)                                                        */
    int32_t value_batches;  /* value minibatches since the last policy reset                                               */
    int32_t reserved0;
    float loss_old;         /* L(theta_old)                                                                                */
    float loss_new;         /* L of the last trial                                                                         */
    float rr_old;           /* CG: r.r of the current direction                                                            */
    float rr;               /* CG: r.r after the last iteration (the final residual)                                       */
    float cg_alpha, cg_beta;
    float xhx;              /* x.F x                                                                                       */
    float step;             /* sqrt(2 max_kl / xhx)                                                                        */
    float expected;         /* g.full, then times alpha_i per trial (skrl's cumulative product)                            */
    float kl;               /* mean KL(theta_old || theta) of the last trial                                               */
    float value_loss_sum;   /* sum of the value minibatch losses since the last policy reset                               */
    float grad_norm;        /* value gradient norm of the last rover_trpo_value_apply, before clipping                     */
    float clip_coef;        /* min(1, max_grad_norm / (grad_norm + 1e-6))                                                  */
    float step_size;        /* (float)(value_lr / (1 - beta1^step))                                                        */
    float bc2_sqrt;         /* (float)sqrt(1 - beta2^step)                                                                 */
    float reserved1;
} rover_trpo_state;

int rover_trpo_default_hparams(rover_trpo_hparams *h);
/* sizeof(rover_trpo_hparams) / sizeof(rover_trpo_state): let a binding check its mirrors of the structs. */
size_t rover_trpo_hparams_bytes(void);
size_t rover_trpo_state_bytes(void);

/* Floats of the flat parameter vector for this policy / value pair; 0 if a descriptor is not the reference pair. */
size_t rover_trpo_param_floats(const rover_policy_desc *policy, const rover_policy_desc *value);
/* Device workspace bytes for a policy step over up to `rows` rows and value minibatches of up to `max_minibatch_rows`
 * rows: the theta_old activation cache (690 floats per row), a scratch of the same size, the chunk partials of the weight
 * gradients and the CG vectors.  The value region is disjoint from the policy region.  0 if an argument is < 1. */
size_t rover_trpo_workspace_bytes(int32_t rows, int32_t max_minibatch_rows);

/* Step 1: resets the state (but value_step), runs the policy forward at theta_old = params over rows 0 .. B of the flat
 * rollout buffers (obs (B, 965), act (B, 2), logp (B), adv (B)), caches its activations and theta_old in `ws`, writes
 * L_old to the state and g = dL/dtheta into `grad` (rover_trpo_param_floats floats, value block zero).  ws: at least
 * rover_trpo_workspace_bytes(B, 1) bytes, 16-byte aligned. */
int rover_trpo_policy_grad(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_trpo_hparams *h,
                           const float *params, const float *obs, const float *act, const float *logp, const float *adv,
                           int32_t B, void *ws, size_t ws_bytes, float *grad, void *state, void *stream);

/* One Fisher-vector product out = F v + damping v at the theta_old cached by the last rover_trpo_policy_grad on this
 * workspace (same params, obs and B).  v / out: rover_trpo_param_floats floats, out's value block written as zeros. */
int rover_trpo_fvp(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_trpo_hparams *h,
                   const float *params, const float *obs, int32_t B, void *ws, size_t ws_bytes, const float *v, float *out,
                   void *stream);

/* Steps 1-5 as one launch sequence: rover_trpo_policy_grad, CG (h->cg_steps iterations at most), the step and the line
 * search (h->max_backtrack trials at most), writing the accepted policy block and log_std into `params` (or restoring
 * theta_old bit for bit), then the n_copies replicas of the policy block rover_policy_forward reads (replicas may be NULL).
 * grad_out (may be NULL) receives g, dir_out (may be NULL) the CG solution x.  The value block of params is not touched. */
int rover_trpo_policy_step(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_trpo_hparams *h,
                           float *params, const float *obs, const float *act, const float *logp, const float *adv, int32_t B,
                           void *ws, size_t ws_bytes, void *state, float *replicas_policy, int32_t n_copies, float *grad_out,
                           float *dir_out, void *stream);

/* One value minibatch: forward of the value network on rows idx[0 .. n) (int64, any order, repeats allowed) of obs (rows,
 * 965) and ret, loss = value_loss_scale mse(ret, V) added to the state's value_loss_sum, and its gradient into the value
 * block of `grad` (only that block is written).  ws: rover_trpo_workspace_bytes(rows, n) bytes or more -- the value region
 * does not disturb the policy cache. */
int rover_trpo_value_minibatch(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_trpo_hparams *h,
                               const float *params, const float *obs, const float *ret, const int64_t *idx, int32_t n,
                               int32_t rows, void *ws, size_t ws_bytes, float *grad, void *state, void *stream);

/* clip_grad_norm_(value, max_grad_norm) and one Adam step (torch's order, lr = value_lr) of the value block of params with
 * the value block of grad and of the moments adam_m / adam_v (full-length vectors, only the value block is read or
 * written); then the n_copies replicas of the value block (may be NULL).  `grad`'s value block is left scaled by the clip
 * coefficient, as torch leaves it.  ws: the workspace of the other calls. */
int rover_trpo_value_apply(const rover_policy_desc *policy, const rover_policy_desc *value, const rover_trpo_hparams *h,
                           float *params, float *grad, float *adam_m, float *adam_v, void *state, float *replicas_value,
                           int32_t n_copies, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_TRPO_H */
