/*
 * rover_td3.h -- C ABI of the fused TD3 update of the rover networks (librover_hip.so).
 *
 * skrl 1.1 TD3._update with the reference's rover_td3.yaml (one gradient step per call pair, batch 4096, actor and critic lr
 * 1e-4, gamma 0.99, polyak 0.005, policy delay 2, no gradient clipping) on:
 *   - the actor (policy and target policy): the reference architecture with no final activation,
 *     rover_policy_default_desc(d, 2, 0) packed by rover_policy_pack;
 *   - the critics (critic_1, critic_2 and their targets): Q(s, a), rover_td3_critic_desc packed by rover_td3_critic_pack.
 *     Encoder 961 -> 80 -> 60 on obs[:, 3:-1] (the reference's one-column-early slice), MLP input [obs[:, 0:4], enc, a]
 *     (4 + 60 + 2 = 66) -> 256 -> 160 -> 128 -> 1, LeakyReLU(0.01).  The MLP's K = 66 does not chain with prop_dim + encoder
 *     output, so rover_policy_pack, rover_policy_forward, rover_ppo_* and rover_trpo_* refuse this descriptor;
 *     rover_policy_unpack reads it as it stands.
 * Any other descriptor returns ROVER_ERR_UNSUPPORTED.
 *
 * One step of skrl's loop is rover_td3_critic_step, then -- on every policy_delay-th critic step, which the host counts --
 * rover_td3_actor_step and rover_td3_polyak on the same sampled rows:
 *   critic: a' = target_policy(s') [; a' = clamp(a' + clamp(noise, -noise_clip, noise_clip), act_min, act_max)],
 *           y = r + (gamma * !terminated) * min(tq1(s', a'), tq2(s', a')), critic_loss = (mse(q1(s, a), y) + mse(q2(s, a), y)) / 2,
 *           one Adam step (critic_lr) over both critics;
 *   actor:  policy_loss = -mean q1(s, pi(s)) with the critic_1 just updated, one Adam step (actor_lr) on the actor;
 *   polyak: target = target * (1 - polyak) + polyak * params over the whole vector (skrl: t.mul_(1 - tau); t.add_(tau * p)),
 *           with tau the float the struct holds, widened to double: see rover_td3_polyak for when that is skrl's result.
 *
 * Parameters live in ONE flat device vector: [actor packed | critic_1 packed | critic_2 packed | zero padding],
 * rover_td3_param_floats() floats.  The target vector, the gradient and both Adam moments have the same layout.
 *
 * Replay memory: an observation ring of `slots` = M + 1 slots x num_envs rows x 965 floats.  Memory slot k (0 .. M) holds
 * act[k] (num_envs, 2), rew[k], terminated[k] (num_envs; terminated as bytes, 0 or 1), its states in ring slot ring_pos[k]
 * and its next_states in ring slot (ring_pos[k] + 1) % slots.  A sampled row index i (int64) is k * num_envs + env; rows
 * i >= valid_rows (the filled part of the memory) or with a ring position outside [0, slots) read row 0 instead and set the
 * state's bad_index word (sticky).  Ring offsets are 64-bit.
 *
 * Conventions as in rover_trpo.h: plain C, caller-owned DEVICE buffers, int return codes, every call asynchronous on `stream`,
 * no host synchronisation, no atomics, -ffp-contract=off.
 *
 * Numerics and reduction order (bit-reproducible from run to run; results are fp32 and agree with float64, not bit for bit
 * with torch -- except rover_td3_polyak, which is bit-identical to torch's fp32 mul_ / add_ for tau = (double)h->polyak):
 *   - dense layers (forward Z = A W^T + b; reverse dA = dZ W) on v_mfma_f32_16x16x4_f32, the reduction over k in ascending
 *     groups of 4 (one MFMA per group); LeakyReLU' from the sign of the stored activation;
 *   - weight / bias gradients dW = sum_rows dZ^T A: rows cut into fixed chunks of 512, one MFMA chain per (tile, chunk) over the
 *     chunk's rows in ascending groups of 4, then the chunk partials added in chunk order;
 *   - per-row terms (squared errors, Q and y means): per 256-row block a fixed halving tree, then one workgroup: thread t adds
 *     block partials t, t + 256, ... in order, then a fixed halving tree;
 *   - Adam in torch's single-tensor order (rover_trpo.h's value Adam without the clip).
 */
#ifndef ROVER_TD3_H
#define ROVER_TD3_H

#include <stddef.h>
#include <stdint.h>

#include "rover_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Hyper-parameters; defaults = skrl TD3_DEFAULT_CONFIG with rover_td3.yaml. */
typedef struct rover_td3_hparams {
    float gamma;                 /* discount_factor (0.99)                                                                 */
    float polyak;                /* 0.005                                                                                  */
    float actor_lr, critic_lr;   /* actor_learning_rate, critic_learning_rate (1e-4, 1e-4)                                 */
    float beta1, beta2, eps;     /* Adam (0.9, 0.999, 1e-8)                                                                */
    float noise_clip;            /* smooth_regularization_clip (0.5), used only when smoothing noise is given              */
    float act_min, act_max;      /* clip_actions_min / max of the smoothed target action (-1, 1)                           */
} rover_td3_hparams;

/* Device-resident state (caller-allocated, 64 bytes, 8-byte aligned, zero it once before the first call). */
typedef struct rover_td3_state {
    int32_t critic_step;         /* critic Adam steps taken                                                                */
    int32_t actor_step;          /* actor Adam steps taken                                                                 */
    int32_t critic_updates;      /* skrl's _critic_update_counter                                                          */
    int32_t bad_index;           /* 1 once a sampled row fell outside the filled memory (never reset by the library)       */
    float critic_loss;           /* (mse(q1, y) + mse(q2, y)) / 2 of the last critic step                                  */
    float policy_loss;           /* -mean q1(s, pi(s)) of the last actor step                                              */
    float q1_mean, q2_mean, y_mean;
    float critic_step_size, critic_bc2_sqrt;   /* (float)(critic_lr / (1 - beta1^t)), (float)sqrt(1 - beta2^t)             */
    float actor_step_size, actor_bc2_sqrt;
    float reserved[3];
} rover_td3_state;

int rover_td3_default_hparams(rover_td3_hparams *h);
/* sizeof(rover_td3_hparams) / sizeof(rover_td3_state): let a binding check its mirrors of the structs. */
size_t rover_td3_hparams_bytes(void);
size_t rover_td3_state_bytes(void);

/* Fills `d` with the critic's Q(s, a) layout (offsets unset until rover_td3_critic_pack). */
int rover_td3_critic_desc(rover_policy_desc *d);
/* Host-side packing of a critic (pure CPU): rover_policy_pack's fragment layout; sets w_off / b_off in `d` and writes
 * rover_policy_packed_floats(d) floats to `packed`.  weights[i] row-major (N, K), biases[i] (N). */
int rover_td3_critic_pack(rover_policy_desc *d, const float *const *weights, const float *const *biases, float *packed);

/* Floats of the flat parameter vector; 0 if `actor` is not rover_policy_default_desc(2, 0) packed by rover_policy_pack or
 * `critic` not rover_td3_critic_desc packed by rover_td3_critic_pack. */
size_t rover_td3_param_floats(const rover_policy_desc *actor, const rover_policy_desc *critic);
/* Device workspace bytes for steps over up to `max_rows` sampled rows; 0 if max_rows < 1. */
size_t rover_td3_workspace_bytes(int32_t max_rows);

/* The critic step over n sampled rows idx[0 .. n): gathers (s, a, r, s', terminated), runs the target actor, the smoothing
 * (noise: (n, 2) floats or NULL = none), both target critics, y, both critics, the loss and its gradient, which it writes into
 * the critic blocks of `grad` (the actor block is not touched), then Adam on the critic blocks of params / adam_m / adam_v.
 * `target` is the target vector.  y_out (n floats, may be NULL) receives y.  ws: rover_td3_workspace_bytes(n) bytes or more,
 * 16-byte aligned, like params and target. */
int rover_td3_critic_step(const rover_policy_desc *actor, const rover_policy_desc *critic, const rover_td3_hparams *h,
                          float *params, const float *target, float *grad, float *adam_m, float *adam_v, const float *obs_ring,
                          int32_t slots, int32_t num_envs, const int32_t *ring_pos, const float *act, const float *rew,
                          const uint8_t *terminated, const int64_t *idx, int32_t n, int64_t valid_rows, const float *noise,
                          void *ws, size_t ws_bytes, void *state, float *y_out, void *stream);

/* The actor step over the same kind of sample: pi(s), critic_1(s, pi(s)), policy_loss, the backward through critic_1's MLP
 * to its two action inputs only (no critic weight gradient, no encoder backward), the actor's backward and weight gradients
 * into the actor block of `grad` (the critic blocks are not touched), Adam on the actor block, then the n_copies replicas of
 * the actor block that rover_policy_forward reads (replicas may be NULL).  dact_out (n x 2 floats, may be NULL) receives
 * d policy_loss / d a at a = pi(s). */
int rover_td3_actor_step(const rover_policy_desc *actor, const rover_policy_desc *critic, const rover_td3_hparams *h,
                         float *params, float *grad, float *adam_m, float *adam_v, const float *obs_ring, int32_t slots,
                         int32_t num_envs, const int32_t *ring_pos, const int64_t *idx, int32_t n, int64_t valid_rows,
                         void *ws, size_t ws_bytes, void *state, float *replicas_actor, int32_t n_copies, float *dact_out,
                         void *stream);

/* target[e] = target[e] * keep then + h->polyak * params[e], for e < count (elementwise: two products and one sum, each
 * rounded to fp32), with keep = (float)(1.0 - (double)h->polyak).  That is bit for bit torch's fp32
 * `t.mul_(1 - tau); t.add_(tau * p)` for the Python float tau = (double)h->polyak, the float32 the struct holds.  skrl forms
 * 1 - tau from the double it was configured with, so its result is the same exactly when
 * (float)(1 - tau_double) == (float)(1 - (double)(float)tau_double): true at the default 0.005, at 0.05 and at 0.25; false at 0.9
 * (0.1 against 0.100000024), 0.99, 0.995, 0.999 and about 40 % of the four-decimal taus in (0, 1), where `keep` is off by up to
 * 2^-25 (half a float32 ulp of tau: several ulps of a small 1 - tau).  polyak = 1 gives keep = 0 and, for finite targets, a
 * copy of params (skrl: t.copy_(p)).  `count`
 * needs no alignment or padding; elements at and past `count` are not touched. */
int rover_td3_polyak(const rover_td3_hparams *h, float *target, const float *params, size_t count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_TD3_H */
