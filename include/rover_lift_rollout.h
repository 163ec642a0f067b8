/*
 * rover_lift_rollout.h -- C ABI of the fused on-policy rollout step of the lift task (librover_hip.so).
 *
 * Replaces, per env step of a PPO rollout on FrankaCubeLift-v0, what a skrl-style trainer does around env.step with the lift
 * task's networks (rover_lift_policy_desc: MLP 36 -> 256 -> 128 -> 64 -> {A, 1}, ELU) and its two RunningStandardScalers
 * (rover_lift_train.h; skrl_ppo_cfg.yaml: clip_actions False, log-std clamp [-20, 2], rewards_shaper_scale 0.01):
 *
 *     s        = clamp((o - (float)mean) / (sqrtf((float)var) + scaler_eps), -scaler_clip, scaler_clip)
 *                                                     (the forward formula of rover_lift_train.h: fp32, no contraction, from
 *                                                      the float64 state-scaler block, which is only read here)
 *     mean, v  = actor(s), critic(s)                  (bit-identical to rover_policy_forward's generic kernel on s)
 *     val      = sqrtf((float)var_v) * clamp(v, -scaler_clip, scaler_clip) + (float)mean_v
 *                                                     (the inverse formula of rover_lift_train.h; v itself without a value scaler)
 *     eps      = N(0, 1) from Philox4x32-10, keyed by (seed, global env id, step counter, action pair)
 *     act      = mean + expf(clamp(log_std)) * eps     (a separate multiply and add)
 *     env_act  = clip_actions ? clamp(act, low, high) : act
 *                (clamp as torch.clamp: a NaN stays NaN; +inf / -inf clamp to high / low)
 *     logp     = sum_c (-0.5 x_c^2 - ls_c - 0.9189385332),  x_c = (act_c - mean_c) / std_c
 *                                                     (the expression rover_lift_ppo_minibatch evaluates for the new policy,
 *                                                      operation for operation: the sum starts at 0 and runs in column order)
 *
 * in ONE launch (rover_lift_rollout_act), and the scaled reward, the done flag and the episode-log tally in a second, small one
 * (rover_lift_rollout_record).
 *
 * The draws are those of rover_rollout.h with a tag of their own: row r of a call has the global id g = env_id_offset + r, and
 * the normal pair p = c / 2 of step `counter` comes from
 *     w = Philox4x32-10(counter = (g, counter & 0xffffffff, counter >> 32, 0x4C524F00 | p), key = (seed_lo, seed_hi))
 *     u1 = ((w0 >> 9) + 0.5) * 2^-23,  u2 = ((w1 >> 9) + 0.5) * 2^-23        (exact in fp32, strictly inside (0, 1))
 *     rho = sqrt(-2 ln u1),  eps[2p] = rho cos(2 pi u2),  eps[2p + 1] = rho sin(2 pi u2)
 * (w2, w3 unused; an odd action width uses the cosine of its last pair).  The values depend on (seed, g, counter, c) only: not on
 * how the envs are split over calls or ranks, and a checkpoint is the counter.  Word 3 of the lift env's own draws is 0 (the
 * reset draw, and the command draw of a reset) or 1 + k (the k-th timer resample of the command since the env's last reset,
 * rover_lift.h: k stays far below this tag, which it would take 1.28e9 resamples within one episode to reach) and word 3 of the
 * rover collector's draws is 0x524F4C00 | p, so the three streams never meet, even under the same seed.
 *
 * Conventions as in rover_rollout.h: plain C, caller-owned device buffers, int return codes, rover_last_error(), asynchronous on
 * `stream`, no allocation, no host synchronisation, no atomics.
 */
#ifndef ROVER_LIFT_ROLLOUT_H
#define ROVER_LIFT_ROLLOUT_H

#include <stddef.h>
#include <stdint.h>

#include "rover_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rover_lift_rollout_hparams {
    uint32_t seed_lo, seed_hi;        /* Philox key */
    int32_t  env_id_offset;           /* global id of row 0 (LiftEnvCfg.env_id_offset) */
    int32_t  clip_actions;            /* 1: env_act = clamp(act, action_low, action_high); skrl_ppo_cfg.yaml: False */
    float    action_low, action_high; /* -1, 1; action_low > action_high is only refused when clip_actions is set */
    float    log_std_min, log_std_max;/* -20, 2 */
    float    scaler_eps, scaler_clip; /* RunningStandardScaler epsilon and clip_threshold (1e-8, 5) */
    float    reward_scale;            /* rewards_shaper_scale (0.01): the caller passes it on to rover_lift_rollout_record */
} rover_lift_rollout_hparams;

/* seed 42 (seed_lo = 42, seed_hi = 0), env_id_offset 0, clip_actions 0, [-1, 1], [-20, 2], 1e-8, 5, 0.01 */
int    rover_lift_rollout_default_hparams(rover_lift_rollout_hparams *h);
size_t rover_lift_rollout_hparams_bytes(void);

/* One launch over rows [0, n) of `obs` (n, 36), 16 rows per workgroup.
 *   state_scaler (73 doubles) the state scaler's block (rover_lift_train.h), 8-byte aligned, read only
 *   value_scaler (3 doubles)  the value scaler's block, or NULL: val_out is then the raw critic output
 *   obs_out     (n, 36)   the RAW rows (the update standardises rows itself); may be NULL; must not alias `obs` (ROVER_ERR_INVALID)
 *   mean_out    (n, A)    A = actor->layers[3].N <= 16    } bit-identical to rover_policy_forward (generic kernel) on the rows
 *   val_out     (n, 1)                                    } rover_lift_ppo_standardize makes of `obs`, then the inverse value scaler
 *   act_out     (n, A)    mean + std * eps
 *   env_act_out (n, A)    what env.step takes
 *   logp_out    (n)       the row's log-probability
 *   eps_out     (n, A)    the standard normal draws
 * act_out, env_act_out, logp_out and eps_out may each be NULL; with all four NULL no draw is made (the bootstrap-value call after
 * the last step).  `log_std` is a DEVICE pointer to A floats (the raw, unclamped parameter: a live view into the trainer's flat
 * parameter vector works as it is).  `actor` / `critic` must be rover_lift_policy_desc(A <= 16) / (1) as rover_policy_pack lays
 * them out (ROVER_ERR_UNSUPPORTED otherwise: the rover's networks have rover_rollout.h); `packed_a` / `packed_b` as in
 * rover_policy_forward (16-byte aligned, n_copies replicas; workgroup b reads replica b % n_copies). */
int rover_lift_rollout_act(const rover_policy_desc *actor, const float *packed_a,
                           const rover_policy_desc *critic, const float *packed_b, int32_t n_copies,
                           const rover_lift_rollout_hparams *h, uint64_t counter,
                           const float *obs, int32_t n, const float *log_std,
                           const double *state_scaler, const double *value_scaler,
                           float *obs_out, float *mean_out, float *val_out,
                           float *act_out, float *env_act_out, float *logp_out, float *eps_out, void *stream);

/* rew_out[i] = rew[i] * reward_scale, done_out[i] = (terminated[i] | truncated[i]) ? 1.0f : 0.0f for i < n.  When `log` (the lift
 * env's device log vector: log[0 .. 5] the mean episode reward terms and log[6 .. 7] the termination counts of the envs that were
 * reset in this step, log[8] their number k) is not NULL, one thread also tallies the episodes: if k > 0,
 *     ep_sum[j] += log[j] * (j < 6 ? k : 1)  for j < 8,    ep_count[0] += k
 * (a product, then a sum; plain loads and stores).  ep_sum (8 floats) / ep_count (1 float) are required with `log` only. */
int rover_lift_rollout_record(const float *rew, const uint8_t *terminated, const uint8_t *truncated, int32_t n,
                              float reward_scale, const float *log, float *rew_out, float *done_out,
                              float *ep_sum, float *ep_count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_LIFT_ROLLOUT_H */
