/*
 * rover_sac_collect.h -- C ABI of the fused SAC transition collector (librover_hip.so).
 *
 * Replaces, per env step of a SAC loop, what a trainer does around env.step (skrl's SAC.act on the Gaussian policy,
 * record_transition into the memory, RandomMemory.sample's indices and the update's standard normal draws; the torch loop of
 * examples/09_train_sac.py):
 *
 *     mu       = tanh(actor(ring[cursor]))                                  (exactly rover_policy_forward on the tanh actor)
 *     sigma    = exp(clamp(log_std, -20, 2))
 *     eps      = N(0, 1) from Philox4x32-10, keyed by (seed, global env id, counter, action pair)
 *     act      = clamp(mu + sigma * eps, -1, 1);  logp = sum_c(-0.5 t_c^2 - ls_c - ln(2 pi) / 2),  t = (act - mu) / sigma
 *     env.step(act)
 *     ring[cursor + 1] = nan_to_num(raw_obs, nan=0, posinf=FLT_MAX, neginf=0);  rewards[k], terminated[k], ring_pos[k]
 *     idx[i]   = uniform row index in [0, mem_rows) from Philox4x32-10, keyed by (seed, counter, i)
 *     eps'[i]  = four standard normals per batch position for the update (rover_sac.h: columns 0:2 for s', 2:4 for s)
 *
 * in TWO launches: rover_sac_collect_act before env.step, rover_sac_collect_record after it.  Nothing is written from the host.
 * The TD3 collector (rover_td3_collect.h) cannot stand in: its actor has no final activation and no log_std, and its exploration
 * is additive noise under a schedule, where SAC samples from the policy's own Gaussian head.
 *
 * Every draw is counter-based, Philox4x32-10 under key = (seed_lo, seed_hi), with a word-3 tag of its own.  The tags of this
 * repository, none of which shares its upper 24 bits with another (the low 8 bits carry an action pair or quad):
 *     0, 1, 2                    the env's own draws                      (rover_hip.h)
 *     0x524F4C00 | pair          the rollout collector's actions          (rover_rollout.h)
 *     0x4C524F00 | pair          the lift rollout collector's actions     (rover_lift_rollout.h)
 *     0x54443300 | pair          TD3 exploration noise, GAUSSIAN and OU   (rover_td3_collect.h)
 *     0x54335300                 TD3 and SAC batch row indices            (rover_td3_collect.h, here)
 *     0x54335200 | quad          ROVER_TD3_TAG_RANDOM: RANDOM's uniforms  (rover_td3_explore.h)
 *     0x54334E00 | pair          ROVER_TD3_TAG_SMOOTH: TD3's smoothing noise and SAC's update draws (rover_td3_explore.h, here)
 *     0x53414300 | pair          ROVER_SAC_TAG_ACTION: SAC's action draws (here)
 *     0x53415200 | quad          ROVER_SAC_TAG_RANDOM: SAC's random steps (here)
 * Action draws: row r of a call has the global id g = env_id_offset + r (formed in unsigned arithmetic), and the normal pair
 * p = c / 2 comes from
 *     w = Philox4x32-10(counter = (g, counter & 0xffffffff, counter >> 32, ROVER_SAC_TAG_ACTION | p), key = (seed_lo, seed_hi))
 * with the uniforms, the Box-Muller form and sincospif exactly as in rover_rollout.h (u = ((w >> 9) + 0.5) * 2^-23 of w0 / w1,
 * rho = sqrt(-2 ln u1), eps[2p] = rho cos(2 pi u2), eps[2p + 1] = rho sin(2 pi u2)).
 *
 * Two streams are REUSED on purpose.  The batch indices are the TD3 collector's (tag 0x54335300: position i takes word i & 3 of
 * the block (i >> 2, counter, tag), index = (word * mem_rows) >> 32), and the update's draws are exactly
 * rover_td3_smooth_draw(seed, counter, std = 1, n = batch, A = 4) (tag ROVER_TD3_TAG_SMOOTH | (c >> 1), counter block (i, counter,
 * tag)).  So the two outputs are bit-comparable with kernels already pinned on hardware, and their specification is
 * td3_collect.sample_indices and td3_explore.smooth_normals as they stand.  A process that runs a TD3 and a SAC collector under one
 * seed and one counter sees the same indices in both; give them different seeds if that matters.
 *
 * Conventions as in rover_td3_collect.h: plain C, caller-owned device buffers, int return codes, rover_last_error(), asynchronous
 * on `stream`, no allocation, no host synchronisation; bad arguments are refused without a launch.
 */
#ifndef ROVER_SAC_COLLECT_H
#define ROVER_SAC_COLLECT_H

#include <stddef.h>
#include <stdint.h>

#include "rover_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ROVER_SAC_COLLECT_SAMPLE 0   /* act = clamp(mu + sigma eps, -1, 1), with its log-probability */
#define ROVER_SAC_COLLECT_MEAN   1   /* act = mu: evaluation */
#define ROVER_SAC_COLLECT_RANDOM 2   /* act uniform in (-1, 1): skrl's random_timesteps */

#define ROVER_SAC_TAG_ACTION 0x53414300u   /* "SAC\0" | action pair */
#define ROVER_SAC_TAG_RANDOM 0x53415200u   /* "SAR\0" | action quad */

typedef struct rover_sac_collect_hparams {
    uint32_t seed_lo, seed_hi;        /* Philox key */
    int32_t  env_id_offset;           /* global id of row 0 (RoverEnvCfg.env_id_offset) */
    int32_t  mode;                    /* ROVER_SAC_COLLECT_*; rover_sac_collect_record does not read it */
} rover_sac_collect_hparams;

/* seed 42 (seed_lo = 42, seed_hi = 0), env_id_offset 0, mode SAMPLE */
int    rover_sac_collect_default_hparams(rover_sac_collect_hparams *h);
size_t rover_sac_collect_hparams_bytes(void);

/* One launch over rows [0, n) of `obs` (n, 965), already sanitised (a ring slot).  The action width is 2 and the action bounds are
 * [-1, 1], as rover_sac.h's Gaussian head has them.
 *
 * SAMPLE and MEAN: 16 rows per 512-thread workgroup; the network part is the TD3 collector's (the same device function), the last
 * layer's sum plus bias y goes through the epilogue below on the lanes that hold it.
 *   mean_out    (n, 2)  mu = tanh(y), bit-identical to rover_policy_forward on the same rows; may be NULL
 *   act_out     (n, 2)  the memory's action slot   } the same values
 *   env_act_out (n, 2)  what env.step takes        }
 *   eps_out     (n, 2)  the standard normal draws; may be NULL; untouched in MEAN
 *   logp_out    (n)     the log-probability of the CLAMPED action; may be NULL; untouched in MEAN
 *   sigma_out   (2)     exp(clamp(log_std)); may be NULL; written by one lane of workgroup 0; untouched in MEAN
 *   log_std     (2)     device pointer, read by the kernel at every launch (FusedSAC.log_std); required in SAMPLE, not read otherwise
 * SAMPLE, per row and column c, every step a separate fp32 operation in this order, nothing contracted into an FMA, both clamps
 * those of torch.clamp (a NaN stays NaN), tanh / exp the Cephes sequences of rover_policy_forward and rover_sac.h:
 *     mu = tanh(y);  ls = clamp(log_std[c], -20, 2);  sigma = exp(ls)
 *     s = sigma * eps;  x = mu + s;  u = clamp(x, -1, 1)
 *     t = (u - mu) / sigma;  term_c = (-0.5f * (t * t) - ls) - 0.918938533f
 *     logp = term_0 + term_1
 * which is the order of rover_sac.h's Gaussian head.  MEAN: act = mu, no draw.
 *
 * RANDOM: a kernel of its own with no LDS; the actor is not evaluated, `packed` and `log_std` are not read (actor and packed must
 * still be valid arguments); mean_out, eps_out, logp_out and sigma_out are untouched.  For row r (g = env_id_offset + r), column c:
 *     w = word c & 3 of Philox4x32-10(counter = (g, counter & 0xffffffff, counter >> 32, ROVER_SAC_TAG_RANDOM | (c >> 2)), key)
 *     u = ((w >> 9) + 0.5) * 2^-23                       (exact, inside (0, 1))
 *     act = -1 + 2 * u                                   (a product and a sum, each rounded to fp32)
 *
 * `actor` must be the reference architecture with two tanh outputs (ROVER_ERR_UNSUPPORTED otherwise); `packed` as in
 * rover_policy_forward (16-byte aligned, n_copies replicas).  An unknown mode is ROVER_ERR_INVALID. */
int rover_sac_collect_act(const rover_policy_desc *actor, const float *packed, int32_t n_copies, const float *log_std,
                          const rover_sac_collect_hparams *h, uint64_t counter,
                          const float *obs, int32_t n,
                          float *mean_out, float *act_out, float *env_act_out, float *eps_out, float *logp_out, float *sigma_out,
                          void *stream);

/* One launch: rover_td3_collect_record's contract, argument for argument, plus eps_out.
 *   ring_slot_out[j] = nan_to_num(obs_raw[j], nan = 0, posinf = FLT_MAX, neginf = 0) for j < n * 965 (bit-exact with torch;
 *                      16-byte pieces when both pointers are 16-byte aligned, scalar otherwise)
 *   rew_out[i] = rew[i], term_out[i] = terminated[i] != 0 for i < n        (rew, terminated, rew_out, term_out: all or none NULL)
 *   *ring_pos_entry = ring_pos_value                                        (one lane; ring_pos_entry may be NULL)
 *   idx_out[i] for i < batch, the TD3 collector's indices                   (idx_out may be NULL: `mem_rows` is unused then)
 *   eps_out[i][0 .. 3] for i < batch, rover_td3_smooth_draw's values at std = 1 and A = 4, one 16-byte store per position
 *                                                                           (eps_out may be NULL; it must be 16-byte aligned)
 * `batch` and `h` are read when idx_out or eps_out is given.  With every record pointer NULL only the rows go in (the rows after a
 * reset).  ring_slot_out must not alias obs_raw, and mem_rows must lie in [1, 2^32] when indices are asked for (ROVER_ERR_INVALID
 * otherwise, without a launch). */
int rover_sac_collect_record(const float *obs_raw, int32_t n, float *ring_slot_out,
                             const float *rew, const uint8_t *terminated, float *rew_out, uint8_t *term_out,
                             int32_t *ring_pos_entry, int32_t ring_pos_value,
                             int64_t *idx_out, int32_t batch, int64_t mem_rows, float *eps_out,
                             const rover_sac_collect_hparams *h, uint64_t counter, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_SAC_COLLECT_H */
