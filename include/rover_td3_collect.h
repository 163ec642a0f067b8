/*
 * rover_td3_collect.h -- C ABI of the fused TD3 transition collector (librover_hip.so).
 *
 * Replaces, per env step of an off-policy (TD3) loop, what a trainer does around env.step (skrl's TD3.act with Gaussian
 * exploration noise, record_transition into the memory, RandomMemory.sample's indices; isaac_rover_orbit_amd/td3.py: explore,
 * ReplayMemory.add, sample_indices):
 *
 *     mean     = actor(ring[cursor])                                       (exactly rover_policy_forward)
 *     eps      = N(0, 1) from Philox4x32-10, keyed by (seed, global env id, counter, action pair)
 *     act      = explore ? clamp(mean + (noise_std * eps) * noise_scale, low, high) : mean
 *                (clamp as torch.clamp: a NaN sum stays NaN, it does not become `low`; +inf / -inf clamp to high / low)
 *     env.step(act)
 *     ring[cursor + 1] = nan_to_num(raw_obs, nan=0, posinf=FLT_MAX, neginf=0);  rewards[k], terminated[k], ring_pos[k]
 *     idx[i]   = uniform row index in [0, mem_rows) from Philox4x32-10, keyed by (seed, counter, i)
 *
 * in TWO launches: rover_td3_collect_act before env.step, rover_td3_collect_record after it.  Nothing is written from the host.
 *
 * The draws are counter-based.  Noise: row r of a call has the global id g = env_id_offset + r, and the normal pair p = c / 2 comes
 * from
 *     w = Philox4x32-10(counter = (g, counter & 0xffffffff, counter >> 32, 0x54443300 | p), key = (seed_lo, seed_hi))
 * with the uniforms, the Box-Muller form and sincospif exactly as in rover_rollout.h (u = ((w >> 9) + 0.5) * 2^-23 of w0 / w1,
 * rho = sqrt(-2 ln u1), eps[2p] = rho cos(2 pi u2), eps[2p + 1] = rho sin(2 pi u2)).  Indices: position i takes word i & 3 of
 *     w = Philox4x32-10(counter = (i >> 2, counter & 0xffffffff, counter >> 32, 0x54335300), key = (seed_lo, seed_hi))
 * and the index is (uint64(word) * mem_rows) >> 32.  The noise depends on (seed, g, counter, c) only and the indices on (seed,
 * counter, i, mem_rows) only: not on tensor shapes or on how the envs are split over calls or ranks, and a checkpoint is the
 * counter.  Word 3 of the env's own draws is 0, 1 or 2 (rover_hip.h), the rollout collectors' are 0x524F4C00 | p and
 * 0x4C524F00 | p (rover_rollout.h, rover_lift_rollout.h): the streams never meet, even under one seed.
 *
 * Conventions as in rover_rollout.h: plain C, caller-owned device buffers, int return codes, rover_last_error(), asynchronous on
 * `stream`, no allocation, no host synchronisation.
 */
#ifndef ROVER_TD3_COLLECT_H
#define ROVER_TD3_COLLECT_H

#include <stddef.h>
#include <stdint.h>

#include "rover_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rover_td3_collect_hparams {
    uint32_t seed_lo, seed_hi;        /* Philox key */
    int32_t  env_id_offset;           /* global id of row 0 (RoverEnvCfg.env_id_offset) */
    int32_t  explore;                 /* 1: noise is drawn and added, the result clamped; 0: act = mean, no draw, no clamp */
    float    noise_std;               /* std of the Gaussian exploration noise */
    float    noise_scale;             /* skrl's linear schedule value (td3.exploration_scale) */
    float    action_low, action_high; /* -1, 1; action_low > action_high is only refused when explore is set */
} rover_td3_collect_hparams;

/* seed 42 (seed_lo = 42, seed_hi = 0), env_id_offset 0, explore 0, noise_std 0, noise_scale 1, [-1, 1] */
int    rover_td3_collect_default_hparams(rover_td3_collect_hparams *h);
size_t rover_td3_collect_hparams_bytes(void);

/* One launch over rows [0, n) of `obs` (n, 965), 16 rows per workgroup.  The rows are ALREADY sanitised (a ring slot).
 *   mean_out    (n, A)  A = actor->layers[5].N <= 16; bit-identical to rover_policy_forward on the same rows; may be NULL
 *   act_out     (n, A)  the memory's action slot   } the same values:
 *   env_act_out (n, A)  what env.step takes        } explore ? clamp(mean + (noise_std * eps) * noise_scale, low, high) : mean
 *   eps_out     (n, A)  the standard normal draws; may be NULL; untouched when explore = 0
 * noise_std * eps, the product with noise_scale and the sum with mean are three separate fp32 operations in that order
 * (td3.explore).  `actor` must be the reference architecture with no final activation (ROVER_ERR_UNSUPPORTED otherwise);
 * `packed` as in rover_policy_forward (16-byte aligned, n_copies replicas). */
int rover_td3_collect_act(const rover_policy_desc *actor, const float *packed, int32_t n_copies,
                          const rover_td3_collect_hparams *h, uint64_t counter,
                          const float *obs, int32_t n,
                          float *mean_out, float *act_out, float *env_act_out, float *eps_out, void *stream);

/* One launch:
 *   ring_slot_out[j] = nan_to_num(obs_raw[j], nan = 0, posinf = FLT_MAX, neginf = 0) for j < n * 965 (bit-exact with torch;
 *                      16-byte pieces when both pointers are 16-byte aligned, scalar otherwise)
 *   rew_out[i] = rew[i], term_out[i] = terminated[i] != 0 for i < n        (rew, terminated, rew_out, term_out: all or none NULL)
 *   *ring_pos_entry = ring_pos_value                                        (one lane; ring_pos_entry may be NULL)
 *   idx_out[i] for i < batch as above                                       (idx_out may be NULL: `batch`, `mem_rows`, `h` unused)
 * With every record pointer NULL only the rows go in (the rows after a reset).  ring_slot_out must not alias obs_raw, and mem_rows
 * must lie in [1, 2^32] when indices are asked for (ROVER_ERR_INVALID otherwise, without a launch). */
int rover_td3_collect_record(const float *obs_raw, int32_t n, float *ring_slot_out,
                             const float *rew, const uint8_t *terminated, float *rew_out, uint8_t *term_out,
                             int32_t *ring_pos_entry, int32_t ring_pos_value,
                             int64_t *idx_out, int32_t batch, int64_t mem_rows,
                             const rover_td3_collect_hparams *h, uint64_t counter, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_TD3_COLLECT_H */
