/*
 * rover_sac.h -- C ABI of the fused SAC update of the rover networks (librover_hip.so).
 *
 * skrl 1.1 SAC._update with the reference's rover_sac.yaml (one gradient step per call, batch 4096, actor and critic lr 1e-4,
 * entropy lr 5e-3, gamma 0.99, polyak 0.005, learned entropy coefficient starting at 0.2, target entropy -2, no gradient
 * clipping) on:
 *   - the policy: the reference's Gaussian actor, tanh on the mean and a state-independent log_std_parameter (2 floats),
 *     rover_policy_default_desc(d, 2, 1) packed by rover_policy_pack.  There is no target policy;
 *   - the critics (critic_1, critic_2 and their targets): Q(s, a), rover_td3_critic_desc packed by rover_td3_critic_pack
 *     (rover_td3.h).
 * Any other descriptor returns ROVER_ERR_UNSUPPORTED.
 *
 * The policy's act (skrl GaussianMixin.act with clip_actions, clip_log_std in [-20, 2], reduction "sum") on a GIVEN standard
 * normal draw eps (2 floats per row):
 *   mu = tanh(z6), ls = clamp(log_std_parameter, -20, 2), sigma = exp(ls), x = mu + sigma * eps, u = clamp(x, -1, 1),
 *   logp = sum_c (-0.5 * ((u - mu) / sigma)^2 - ls - 0.5 * ln(2 pi))        -- the log-probability of the CLAMPED action.
 * Both clamps keep a NaN, as torch.clamp does.
 *
 * One step of skrl's loop is rover_sac_critic_step, rover_sac_policy_step and rover_sac_polyak on the same sampled rows, with
 * eps (n, 4): columns 0, 1 are the draw for s', columns 2, 3 the draw for s:
 *   critic:  (u', logp') = act(s', eps[:, 0:2]),
 *            y = r + (gamma * !terminated) * (min(tq1(s', u'), tq2(s', u')) - alpha * logp'),
 *            critic_loss = (mse(q1(s, a), y) + mse(q2(s, a), y)) / 2, one Adam step (critic_lr) over both critics;
 *   policy:  (u, logp) = act(s, eps[:, 2:4]), policy_loss = mean(alpha * logp - min(q1(s, u), q2(s, u))) with the critics just
 *            updated, one Adam step (actor_lr) over the policy's weights and log_std_parameter; min is torch.min: on an exact
 *            tie half of the gradient goes each way.  Then, with learn_entropy != 0, the entropy step:
 *            entropy_loss = -mean(log_alpha * (logp + target_entropy)) with logp a constant, one Adam step (entropy_lr) on
 *            log_alpha.  alpha = exp(log_alpha) is formed ON THE DEVICE from the parameter vector wherever it is used, as
 *            (float)exp((double)log_alpha); both steps of one update use the alpha from before that update's entropy step;
 *   polyak:  target = target * (1 - polyak) + polyak * params over both critics (skrl: t.mul_(1 - tau); t.add_(tau * p)).
 *
 * Parameters live in ONE flat device vector, rover_sac_param_floats() floats:
 *   [actor packed | critic_1 packed | critic_2 packed | log_std (2 + 2 zero pad) | log_alpha (1 + 3 zero pad) | zero padding to
 *    a multiple of 64 floats].
 * The gradient and both Adam moments have the same layout; the padding's gradient is written as exact zeros.  The target
 * vector holds [critic_1 packed | critic_2 packed] only.
 *
 * Replay memory: rover_td3.h's observation ring and flat row indices; rows outside the filled memory read row 0 and set the
 * state's bad_index word (sticky).
 *
 * Conventions as in rover_td3.h: plain C, caller-owned DEVICE buffers, int return codes, every call asynchronous on `stream`,
 * no host synchronisation, no atomics, -ffp-contract=off.
 *
 * Numerics and reduction order (bit-reproducible from run to run; results are fp32 and agree with float64, not bit for bit
 * with torch -- except rover_sac_polyak, which is bit-identical to torch's fp32 mul_ / add_ for tau = (double)h->polyak):
 *   - dense layers (forward Z = A W^T + b; reverse dA = dZ W) on v_mfma_f32_16x16x4_f32, the reduction over k in ascending
 *     groups of 4 (one MFMA per group); LeakyReLU' from the sign of the stored activation;
 *   - weight / bias gradients dW = sum_rows dZ^T A: rows cut into fixed chunks of 512, one MFMA chain per (tile, chunk) over the
 *     chunk's rows in ascending groups of 4, then the chunk partials added in chunk order;
 *   - per-row terms (squared errors, Q, y and logp means, the policy loss, the log_std gradient): per 256-row block a fixed
 *     halving tree, then one workgroup: thread t adds block partials t, t + 256, ... in order, then a fixed halving tree;
 *   - tanh and exp of the Gaussian head as the explicit fp32 sequences of rover_policy.h's forward;
 *   - Adam in torch's single-tensor order.
 */
#ifndef ROVER_SAC_H
#define ROVER_SAC_H

#include <stddef.h>
#include <stdint.h>

#include "rover_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Hyper-parameters; defaults = skrl SAC_DEFAULT_CONFIG with rover_sac.yaml. */
typedef struct rover_sac_hparams {
    float gamma;                 /* discount_factor (0.99)                                                                 */
    float polyak;                /* 0.005                                                                                  */
    float actor_lr, critic_lr;   /* actor_learning_rate, critic_learning_rate (1e-4, 1e-4)                                 */
    float entropy_lr;            /* entropy_learning_rate (5e-3)                                                           */
    float beta1, beta2, eps;     /* Adam (0.9, 0.999, 1e-8)                                                                */
    float target_entropy;        /* skrl's None: minus the action width (-2)                                               */
    int32_t learn_entropy;       /* 1; 0: log_alpha is never stepped                                                       */
} rover_sac_hparams;

/* Device-resident state (caller-allocated, 80 bytes, 8-byte aligned, zero it once before the first call). */
typedef struct rover_sac_state {
    int32_t critic_step;         /* critic Adam steps taken                                                                */
    int32_t actor_step;          /* policy Adam steps taken                                                                */
    int32_t entropy_step;        /* log_alpha Adam steps taken                                                             */
    int32_t bad_index;           /* 1 once a sampled row fell outside the filled memory (never reset by the library)       */
    float critic_loss;           /* (mse(q1, y) + mse(q2, y)) / 2 of the last critic step                                  */
    float policy_loss;           /* mean(alpha * logp - min(q1, q2)) of the last policy step                               */
    float entropy_loss;          /* -log_alpha * mean(logp + target_entropy) of the last entropy step                      */
    float q1_mean, q2_mean, y_mean;            /* of the last critic step                                                  */
    float logp_mean;             /* mean logp of the last policy step                                                      */
    float alpha;                 /* the entropy coefficient the last policy step used                                      */
    float critic_step_size, critic_bc2_sqrt;   /* (float)(critic_lr / (1 - beta1^t)), (float)sqrt(1 - beta2^t)             */
    float actor_step_size, actor_bc2_sqrt;
    float entropy_step_size, entropy_bc2_sqrt;
    float reserved[2];
} rover_sac_state;

int rover_sac_default_hparams(rover_sac_hparams *h);
/* sizeof(rover_sac_hparams) / sizeof(rover_sac_state): let a binding check its mirrors of the structs. */
size_t rover_sac_hparams_bytes(void);
size_t rover_sac_state_bytes(void);

/* Floats of the flat parameter vector; 0 if `actor` is not rover_policy_default_desc(2, 1) packed by rover_policy_pack or
 * `critic` not rover_td3_critic_desc packed by rover_td3_critic_pack.  log_std sits at
 * packed(actor) + 2 * packed(critic), log_alpha 4 floats after it. */
size_t rover_sac_param_floats(const rover_policy_desc *actor, const rover_policy_desc *critic);
/* Device workspace bytes for steps over up to `max_rows` sampled rows; 0 if max_rows < 1. */
size_t rover_sac_workspace_bytes(int32_t max_rows);

/* The critic step over n sampled rows idx[0 .. n): gathers (s, a, r, s', terminated), runs the policy and its Gaussian head on
 * s' with eps[r * 4 + 0 .. 2), both target critics, y, both critics, the loss and its gradient, which it writes into the critic
 * blocks of `grad` (nothing else of `grad` is touched), then Adam on the critic blocks of params / adam_m / adam_v.  `target`
 * is the target vector [critic_1 | critic_2].  y_out (n floats, may be NULL) receives y.  ws: rover_sac_workspace_bytes(n)
 * bytes or more, 16-byte aligned, like params, target, grad and the moments. */
int rover_sac_critic_step(const rover_policy_desc *actor, const rover_policy_desc *critic, const rover_sac_hparams *h,
                          float *params, const float *target, float *grad, float *adam_m, float *adam_v, const float *obs_ring,
                          int32_t slots, int32_t num_envs, const int32_t *ring_pos, const float *act, const float *rew,
                          const uint8_t *terminated, const int64_t *idx, int32_t n, int64_t valid_rows, const float *eps,
                          void *ws, size_t ws_bytes, void *state, float *y_out, void *stream);

/* The policy step, then the entropy step, over the same kind of sample: the policy and its Gaussian head on s with
 * eps[r * 4 + 2 .. 4), both critics on (s, u), the reverse through both critics' MLPs to their two action inputs only (no critic
 * weight gradient, no encoder reverse), the Gaussian head's closed-form backward, the actor's reverse and weight gradients.
 * Writes the actor block, log_std, log_alpha and the padding of `grad` (the critic blocks are not touched), then Adam on the
 * actor block and log_std (actor_lr) and, with learn_entropy, on log_alpha (entropy_lr), then the n_copies replicas of the
 * actor block that rover_policy_forward reads (replicas may be NULL).  Debug outputs, each may be NULL: u_out (n, 2) the
 * clamped action, logp_out (n), dmean_out (n, 2) = d policy_loss / d mu. */
int rover_sac_policy_step(const rover_policy_desc *actor, const rover_policy_desc *critic, const rover_sac_hparams *h,
                          float *params, float *grad, float *adam_m, float *adam_v, const float *obs_ring, int32_t slots,
                          int32_t num_envs, const int32_t *ring_pos, const int64_t *idx, int32_t n, int64_t valid_rows,
                          const float *eps, void *ws, size_t ws_bytes, void *state, float *replicas_actor, int32_t n_copies,
                          float *u_out, float *logp_out, float *dmean_out, void *stream);

/* target[e] = target[e] * keep then + h->polyak * critics[e] over both critic blocks, critics = params + packed(actor)
 * (elementwise: two products and one sum, each rounded to fp32), with keep = (float)(1.0 - (double)h->polyak): bit for bit
 * torch's fp32 `t.mul_(1 - tau); t.add_(tau * p)` for the Python float tau = (double)h->polyak (see rover_td3_polyak for when
 * that is skrl's result; it is at the default 0.005).  Nothing past the two blocks of `target` is written. */
int rover_sac_polyak(const rover_policy_desc *actor, const rover_policy_desc *critic, const rover_sac_hparams *h, float *target,
                     const float *params, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_SAC_H */
