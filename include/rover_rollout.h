/*
 * rover_rollout.h -- C ABI of the fused on-policy rollout step (librover_hip.so).
 *
 * Replaces, per env step of a PPO / TRPO rollout, what the reference's trainer does around env.step
 * (rover_envs/utils/skrl_utils.py:114-135: agent.act + record_transition; skrl's GaussianMixin.act for the sampling and the
 * log-probability, rover_envs/envs/navigation/learning/skrl/models.py:66 for clip_actions and the log-std clamp):
 *
 *     o        = nan_to_num(raw_obs, nan=0, posinf=FLT_MAX, neginf=0)     (the scanner writes -inf on a miss)
 *     mean, v  = actor(o), critic(o)                                       (exactly rover_policy_forward_pair)
 *     eps      = N(0, 1) from Philox4x32-10, keyed by (seed, global env id, step counter, action pair)
 *     act      = mean + exp(clamp(log_std)) * eps
 *     env_act  = clip_actions ? clamp(act, low, high) : act
 *     logp     = sum_c (-0.5 x_c^2 - ls_c - 0.9189385332),  x_c = (act_c - mean_c) / std_c
 *
 * in ONE launch (rover_rollout_act), and the reward / done record in a second, small one (rover_rollout_record, or
 * rover_rollout_record_shaped with skrl's rewards_shaper_scale and time_limit_bootstrap).
 *
 * The draws are counter-based: row r of a call has the global id g = env_id_offset + r, and the normal pair p = c / 2 of step
 * `counter` comes from
 *     w = Philox4x32-10(counter = (g, counter & 0xffffffff, counter >> 32, 0x524F4C00 | p), key = (seed_lo, seed_hi))
 *     u1 = ((w0 >> 9) + 0.5) * 2^-23,  u2 = ((w1 >> 9) + 0.5) * 2^-23        (exact in fp32, strictly inside (0, 1))
 *     rho = sqrt(-2 ln u1),  eps[2p] = rho cos(2 pi u2),  eps[2p + 1] = rho sin(2 pi u2)
 * (w2, w3 unused; an odd action width uses the cosine of its last pair).  The values depend on (seed, g, counter, c) only: not on
 * how the envs are split over calls or ranks, and a checkpoint is the counter.  Word 3 of the env's own draws is 0, 1 or 2
 * (rover_hip.h), so the streams never meet, even under the same seed.
 *
 * Conventions as in rover_policy.h: plain C, caller-owned device buffers, int return codes, rover_last_error(), asynchronous on
 * `stream`, no allocation, no host synchronisation.
 */
#ifndef ROVER_ROLLOUT_H
#define ROVER_ROLLOUT_H

#include <stddef.h>
#include <stdint.h>

#include "rover_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rover_rollout_hparams {
    uint32_t seed_lo, seed_hi;        /* Philox key */
    int32_t  env_id_offset;           /* global id of row 0 (RoverEnvCfg.env_id_offset) */
    int32_t  clip_actions;            /* 1: env_act = clamp(act, action_low, action_high)  (models.py:66) */
    float    action_low, action_high; /* -1, 1; action_low > action_high is only refused when clip_actions is set */
    float    log_std_min, log_std_max;/* -20, 2 (models.py:66) */
} rover_rollout_hparams;

/* seed 42 (seed_lo = 42, seed_hi = 0), env_id_offset 0, clip_actions 1, [-1, 1], [-20, 2] */
int    rover_rollout_default_hparams(rover_rollout_hparams *h);
size_t rover_rollout_hparams_bytes(void);

/* One launch over rows [0, n) of `obs` (n, 965), 16 rows per workgroup.
 *   obs_out     (n, 965)  the sanitised rows; may be NULL; must not alias `obs` (ROVER_ERR_INVALID)
 *   mean_out    (n, A)    A = actor->layers[5].N <= 16   } bit-identical to rover_policy_forward_pair on the sanitised rows
 *   val_out     (n, B)    B = critic->layers[5].N (1)    }
 *   act_out     (n, A)    mean + std * eps (a separate multiply and add)
 *   env_act_out (n, A)    what env.step takes
 *   logp_out    (n)       the row's log-probability, the expression of rover_ppo_minibatch operation for operation
 *   eps_out     (n, A)    the standard normal draws
 * act_out, env_act_out, logp_out and eps_out may each be NULL; with all four NULL no draw is made (the bootstrap-value call after
 * the last step).  `log_std` is a DEVICE pointer to A floats (the raw, unclamped parameter: a live view into a trainer's flat
 * parameter vector works as it is); std = expf(clamp(log_std, log_std_min, log_std_max)).
 * Both descriptors must be the reference architecture with the same leaky-ReLU slope (ROVER_ERR_UNSUPPORTED otherwise);
 * `packed_a` / `packed_b` as in rover_policy_forward_pair (16-byte aligned, n_copies replicas). */
int rover_rollout_act(const rover_policy_desc *actor, const float *packed_a,
                      const rover_policy_desc *critic, const float *packed_b, int32_t n_copies,
                      const rover_rollout_hparams *h, uint64_t counter,
                      const float *obs, int32_t n, const float *log_std,
                      float *obs_out, float *mean_out, float *val_out,
                      float *act_out, float *env_act_out, float *logp_out, float *eps_out, void *stream);

/* rew_out[i] = rew[i], done_out[i] = (terminated[i] | truncated[i]) ? 1.0f : 0.0f for i < n (one small launch). */
int rover_rollout_record(const float *rew, const uint8_t *terminated, const uint8_t *truncated, int32_t n,
                         float *rew_out, float *done_out, void *stream);

/* rover_rollout_record with skrl's reward shaper and time-limit bootstrap (PPO.record_transition), one launch:
 *     r = rew[i] * reward_scale                                  (rewards_shaper_scale: rover_envs/utils/config.py:84-88)
 *     time_limit_bootstrap != 0:  rew_out[i] = r + (discount * val[i]) * trunc,  trunc = truncated[i] ? 1.0f : 0.0f
 *     time_limit_bootstrap == 0:  rew_out[i] = r                 (val is not read and may be NULL)
 * in fp32, every product and the sum formed (nothing contracted): skrl's `rewards += discount_factor * values * truncated` with
 * `discount` rounded to fp32.  An infinite val on a row that is not truncated gives inf * 0 = NaN, as in torch.  val: THIS step's
 * critic output on the return's scale (the collector's value slot): skrl bootstraps with the value of the pre-step states.
 * done_out as rover_rollout_record.  The float arrays are 4-byte aligned, nothing wider is assumed. */
int rover_rollout_record_shaped(const float *rew, const uint8_t *terminated, const uint8_t *truncated, const float *val, int32_t n,
                                float reward_scale, float discount, int32_t time_limit_bootstrap, float *rew_out, float *done_out,
                                void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_ROLLOUT_H */
