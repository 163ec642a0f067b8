/*
 * rover_td3_explore.h -- C ABI of TD3's exploration switches and smoothing draws (librover_hip.so).
 *
 * rover_td3_collect.h covers skrl's TD3.act at the defaults of rover_td3.yaml: no noise, or Gaussian noise.  This header adds the
 * switches a skrl TD3 user can set besides (isaac_rover_orbit_amd/td3_explore.py: TorchTD3Explorer is the specification):
 *
 *     OFF       act = mean                                                          (rover_td3_collect_act with explore = 0)
 *     GAUSSIAN  act = clamp(mean + (noise_std * eps) * noise_scale, low, high)      (rover_td3_collect_act with explore = 1)
 *     OU        x' = (x - x * theta) + sigma * eps;  act = clamp(mean + (base_scale * x') * noise_scale, low, high);  x <- x'
 *               (skrl's OrnsteinUhlenbeckNoise with a standard normal distribution, one state per env and action column)
 *     RANDOM    act = low + (high - low) * u,  u uniform in (0, 1)                  (skrl's random_act while timestep < random_timesteps)
 *
 * and the draw of the target action's smoothing noise (skrl's smooth_regularization_noise), std * eps per batch position, which
 * rover_td3_critic_step takes as its `noise` argument and clips itself (rover_td3.h).
 *
 * Every draw is counter-based, Philox4x32-10 under key = (seed_lo, seed_hi), with a word-3 tag of its own.  The tags of this
 * repository, none of which shares its upper 24 bits with another (the low 8 bits carry an action pair or quad):
 *     0, 1, 2                    the env's own draws                      (rover_hip.h)
 *     0x524F4C00 | pair          the rollout collector's actions          (rover_rollout.h)
 *     0x4C524F00 | pair          the lift rollout collector's actions     (rover_lift_rollout.h)
 *     0x54443300 | pair          TD3 exploration noise, GAUSSIAN and OU   (rover_td3_collect.h)
 *     0x54335300                 TD3 batch row indices                    (rover_td3_collect.h)
 *     0x54335200 | quad          ROVER_TD3_TAG_RANDOM: RANDOM's uniforms  (here)
 *     0x54334E00 | pair          ROVER_TD3_TAG_SMOOTH: smoothing noise    (here)
 * The exploration draws are indexed by (global env id, counter, action column) and the smoothing draws by (batch position, counter,
 * action column): neither depends on tensor shapes or on how the envs are split over calls or ranks, and a checkpoint is the
 * counter plus, under OU, the state.
 *
 * On skrl: skrl is not a dependency of this project.  The OU recurrence and random_act above are this project's reading of skrl
 * 1.1.0, and the torch specification (td3_explore.TorchTD3Explorer) is the contract.  Two points where that reading and skrl's text
 * may part in the last place or in the draw: skrl writes the OU step as `state += -state * theta + sigma * sample`, which
 * associates as x + ((-x * theta) + sigma * eps), where this contract has (x - x * theta) + sigma * eps: the same real number,
 * rounded in another order.  And skrl draws random_act from the action space's uniform distribution with torch's generator, where
 * this contract draws low + (high - low) * u from Philox.  skrl's OU defaults are theta 0.15, sigma 0.2, base_scale 1.0.
 *
 * Conventions as in rover_td3_collect.h: plain C, caller-owned device buffers, int return codes, rover_last_error(), asynchronous
 * on `stream`, no allocation, no host synchronisation; bad arguments return ROVER_ERR_INVALID without a launch.
 */
#ifndef ROVER_TD3_EXPLORE_H
#define ROVER_TD3_EXPLORE_H

#include <stddef.h>
#include <stdint.h>

#include "rover_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ROVER_TD3_EXPLORE_OFF      0
#define ROVER_TD3_EXPLORE_GAUSSIAN 1
#define ROVER_TD3_EXPLORE_OU       2
#define ROVER_TD3_EXPLORE_RANDOM   3

#define ROVER_TD3_TAG_RANDOM 0x54335200u   /* "T3R\0" | action quad */
#define ROVER_TD3_TAG_SMOOTH 0x54334E00u   /* "T3N\0" | action pair */

typedef struct rover_td3_explore_hparams {
    uint32_t seed_lo, seed_hi;        /* Philox key */
    int32_t  env_id_offset;           /* global id of row 0 (RoverEnvCfg.env_id_offset) */
    int32_t  mode;                    /* ROVER_TD3_EXPLORE_* */
    float    noise_std;               /* GAUSSIAN: std of the noise (OU draws standard normals: it is not read there) */
    float    noise_scale;             /* GAUSSIAN, OU: skrl's linear schedule value (td3.exploration_scale) */
    float    ou_theta, ou_sigma, ou_base_scale;
    float    action_low, action_high; /* -1, 1; action_low > action_high is refused in GAUSSIAN, OU and RANDOM only */
} rover_td3_explore_hparams;

/* seed 42 (seed_lo = 42, seed_hi = 0), env_id_offset 0, mode OFF, noise_std 0, noise_scale 1, theta 0.15, sigma 0.2, base_scale 1,
 * [-1, 1] */
int    rover_td3_explore_default_hparams(rover_td3_explore_hparams *h);
size_t rover_td3_explore_hparams_bytes(void);

/* One launch over rows [0, n) of `obs` (n, 965), already sanitised (a ring slot); A = actor->layers[5].N <= 16.
 *
 * OFF, GAUSSIAN, OU: 16 rows per workgroup and the actor forward of rover_td3_collect_act (the same device function).
 *   mean_out    (n, A)  bit-identical to rover_policy_forward on the same rows; may be NULL
 *   act_out     (n, A)  the memory's action slot   } the same values
 *   env_act_out (n, A)  what env.step takes        }
 *   eps_out     (n, A)  the standard normal draws (tag 0x54443300 | c / 2, as rover_td3_collect_act); may be NULL; untouched in OFF
 *   ou_state    (n, A)  OU only, required there, read and written; in every other mode neither read nor written, may be NULL.
 *                       It is not reset at episode ends (skrl does not reset it).
 *   OFF       exactly rover_td3_collect_act with explore = 0: act = mean, no draw, no clamp.
 *   GAUSSIAN  exactly rover_td3_collect_act with explore = 1: noise = noise_std * eps.
 *   OU        t = x * theta; x1 = x - t; s = sigma * eps; x' = x1 + s; noise = base_scale * x': five separate fp32 operations in this
 *             order; x' goes back to ou_state.
 *   GAUSSIAN and OU then take p = noise * noise_scale, a = mean + p (two more fp32 operations) and the clamp of torch.clamp: a NaN
 *   stays NaN, +inf / -inf clamp to high / low.  Nothing is contracted into an FMA.
 *
 * RANDOM: a kernel of its own with no LDS; the actor is not evaluated and `packed` is not read (actor still gives A, and packed
 * must still be a valid argument); mean_out, eps_out and ou_state are untouched.  For row r (g = env_id_offset + r) and column c,
 *     w = word c & 3 of Philox4x32-10(counter = (g, counter & 0xffffffff, counter >> 32, ROVER_TD3_TAG_RANDOM | (c >> 2)), key)
 *     u = ((w >> 9) + 0.5) * 2^-23                       (exact, inside (0, 1))
 *     act = low + (high - low) * u                       (range = high - low once, then a product and a sum, each rounded to fp32)
 *
 * `actor` must be the reference architecture with no final activation (ROVER_ERR_UNSUPPORTED otherwise); `packed` as in
 * rover_policy_forward (16-byte aligned, n_copies replicas).  An unknown mode is ROVER_ERR_INVALID. */
int rover_td3_explore_act(const rover_policy_desc *actor, const float *packed, int32_t n_copies,
                          const rover_td3_explore_hparams *h, uint64_t counter,
                          const float *obs, int32_t n, float *ou_state,
                          float *mean_out, float *act_out, float *env_act_out, float *eps_out, void *stream);

/* One launch: noise_out[i][c] = std * eps for batch positions i < n and columns c < A, with eps the standard normal of pair c / 2
 * in the Box-Muller / sincospif form of rover_rollout.h (the cosine branch in the even column, the sine branch in the odd one) on
 *     w = Philox4x32-10(counter = (i, counter & 0xffffffff, counter >> 32, ROVER_TD3_TAG_SMOOTH | (c >> 1)), key = (seed_lo, seed_hi)).
 * The values are not clipped: rover_td3_critic_step clips its `noise` argument to h->noise_clip itself, and noise_out is exactly
 * that argument.  n < 1, A odd, A < 2 or A > 16, std < 0 (or NaN) and a NULL noise_out are ROVER_ERR_INVALID. */
int rover_td3_smooth_draw(uint32_t seed_lo, uint32_t seed_hi, uint64_t counter, float std, float *noise_out, int32_t n, int32_t A,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_TD3_EXPLORE_H */
