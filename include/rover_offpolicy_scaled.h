/*
 * rover_offpolicy_scaled.h -- C ABI of the path between the replay ring and a TD3 / SAC update that runs behind skrl's
 * RunningStandardScaler (librover_hip.so).
 *
 * The reference's off-policy agent files (rover_td3.yaml, rover_sac.yaml) list state_preprocessor / state_preprocessor_kwargs as
 * the on-policy ones do; rover_envs/utils/config.py:76-96 turns the entry into skrl's RunningStandardScaler on the 965-wide
 * states.  skrl's TD3._update / SAC._update then standardise the sampled states and next states (and train the statistics on
 * them) before anything else reads them.  The trainers of rover_td3.h / rover_sac.h read their rows from a replay memory
 * (td3.ReplayMemory: an observation ring of slots x num_envs rows plus the transitions), so the scaled update is composed from
 * unchanged parts around a STAGED memory of one slot:
 *
 *   1. rover_offpolicy_stage_resolve   the sampled indices -> ring row numbers of s and s', compact actions / rewards / terminated
 *   2. rover_scaler_train              (rover_scaler.h) on the ring rows of s, read where they lie
 *   3. rover_offpolicy_stage_rows      standardised s  -> staged obs slot 0
 *   4. rover_scaler_train              on the ring rows of s' (a switch of the Python classes)
 *   5. rover_offpolicy_stage_rows      standardised s' -> staged obs slot 1
 *   6. rover_td3_* / rover_sac_*       the unchanged update on the staged memory with the identity index 0 .. n
 *
 * The scaler block, its arithmetic and rover_scaler_hparams are rover_scaler.h's; they are not restated here.
 *
 * Conventions as in rover_scaler.h: plain C, caller-owned DEVICE buffers, int return codes (ROVER_ERR_INVALID for a bad argument),
 * rover_last_error() for the text, every call asynchronous on `stream` and run on the device its first output lives on.  No
 * allocation, no host synchronisation, no atomics.  Row offsets are formed in 64 bit.
 */
#ifndef ROVER_OFFPOLICY_SCALED_H
#define ROVER_OFFPOLICY_SCALED_H

#include <stddef.h>
#include <stdint.h>

#include "rover_scaler.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One launch over the n >= 1 sampled flat indices idx[i] = k * num_envs + env (int64), the rules of the trainers' own gather:
 * an index < 0 or >= valid_rows, or a ring_pos[k] outside [0, slots), reads row 0 (memory slot 0, env 0) resp. ring slot 0 and
 * stores 1 into *bad_index, which no call ever clears (sticky, caller-owned, 4-byte aligned; every writer stores the same word).
 *   rows_s[i]    = ring_pos[k] * num_envs + env                       the ring row of s: rover_scaler_train's idx on the ring
 *   rows_next[i] = ((ring_pos[k] + 1) % slots) * num_envs + env       ... of s'
 *   act_out[i, 0 .. act_dim) = actions[idx[i], :],  rew_out[i] = rewards[idx[i]],  term_out[i] = terminated[idx[i]]   (bit copies;
 *   terminated is one byte per row)
 * valid_rows <= memory slots * num_envs is the caller's to keep (ring_pos holds one entry per memory slot); act_dim in [1, 16]. */
int rover_offpolicy_stage_resolve(const int64_t *idx, int32_t n, int64_t valid_rows, int32_t num_envs, int32_t slots,
                                  const int32_t *ring_pos, const float *actions, int32_t act_dim, const float *rewards,
                                  const uint8_t *terminated, int64_t *rows_s, int64_t *rows_next, float *act_out, float *rew_out,
                                  uint8_t *term_out, int32_t *bad_index, void *stream);

/* One launch: out[i, :] = forward(x[src[i], :]) for i < n, n >= 1; x is (x_rows, width) fp32 row-major (the ring viewed as
 * slots * num_envs rows), src int64, out a compact (n, width) image that does not overlap x (ROVER_ERR_INVALID where the two
 * ranges intersect).  `forward` is rover_scaler_apply's forward expression bit for bit (fp32, no contraction, clamp propagates
 * NaN); the block is not updated.  A repeated src entry is read twice.  A src entry outside [0, x_rows) reads row 0 and stores 1
 * into *bad_index (may be NULL; the rule of rover_offpolicy_stage_resolve).  Words of out past row n are not touched.
 * width in [1, ROVER_SCALER_MAX_WIDTH]; x and out are 4-byte aligned, so a row starts at any 4-byte phase of a 16-byte line and a
 * source row in general at another phase than its destination row.  One wave moves one row: a dword head up to the DESTINATION's
 * 16-byte boundary, then 16-byte stores from 16-byte loads (which are 16-byte aligned only where the two phases agree), then a
 * dword tail.  Every element goes through the same expression whichever piece it falls into: the values do not depend on it. */
int rover_offpolicy_stage_rows(const rover_scaler_hparams *h, const double *scaler, int32_t width, const float *x, int64_t x_rows,
                               const int64_t *src, int32_t n, float *out, int32_t *bad_index, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_OFFPOLICY_SCALED_H */
