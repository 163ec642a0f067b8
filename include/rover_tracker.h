/*
 * rover_tracker.h -- C ABI of skrl's reward / episode tracking kept on the device (librover_hip.so).
 *
 * skrl 1.1.0's Agent.record_transition / track_data / write_tracking_data produce the curves the reference's users watch
 * ("Reward / Instantaneous reward (max|min|mean)", "Reward / Total reward (...)", "Episode / Total timesteps (...)", the
 * "EpisodeInfo / ..." scalars of rover_envs/utils/skrl_utils.py:138-142 and the agents' own "Loss / ...").  Done as skrl does it
 * that is a nonzero(), two tolist() and three item() per env step, each a host synchronisation.  Here the same bookkeeping is two
 * launches per env step on caller-owned device memory and one read-back per write interval.
 *
 * Per step, with rewards r[n], terminated[n], truncated[n] (float32, 0 / 1 as the collectors hold them):
 *     cum_r += r; cum_t += 1; fin = (terminated + truncated) != 0
 *     the finished envs' (cum_r, cum_t), in ascending env id, are appended to two windows of the last 100 episodes
 *     (collections.deque(maxlen=100).extend), then cum_r = cum_t = 0 at the finished envs;
 *     the step's max, min and mean of r, and -- where the windows are not empty -- the max, min and mean of each window are folded
 *     into running accumulators: max of maxes, min of mins, sum of means and a step count.
 * max and min propagate NaN as numpy's do: the result is NaN where any operand is.
 *
 * State block (device memory, 8-byte aligned, rover_tracker_state_bytes(n, slots) bytes), in 4-byte words:
 *     [0] n  [1] slots  [2] head  [3] len  [4] steps  [5] window_steps  [6..7] reserved (0)
 *     [8..13]   double sum[3]     sums of the per-step means: instantaneous reward, total reward, total timesteps
 *     [14..16]  float  max[3]     running max of the per-step maxima (same order); -inf when empty
 *     [17..19]  float  min[3]     running min of the per-step minima; +inf when empty
 *     [20..119]  float   ring_r[100]   total rewards of the last `len` finished episodes; the oldest is at (head - len) mod 100,
 *     [120..219] int32_t ring_t[100]   their lengths;                                   the next one goes to `head`
 *     [220 ..]  double  slot_sum[slots]; int64_t slot_count[slots]; float slot_max[slots]; float slot_min[slots]
 *     then      float   cum_r[n]; int32_t cum_t[n]
 * `steps` counts the steps since the last snapshot, `window_steps` those of them whose windows were not empty.
 *
 * Reduction orders (functions of n alone; the launch boundary is the only synchronisation between workgroups):
 *   instantaneous reward: env e belongs to chunk e / 256, position e % 256; a chunk's 256 values (0.0, -inf, +inf behind n for
 *     the sum, the max and the min) are combined by the tree  x[t] = op(x[t], x[t + s])  for s = 128, 64, ... 1, the sum in
 *     float64.  The chunk results are combined the same way: position t takes the chunks t, t + 256, ... in ascending order onto
 *     0.0 / -inf / +inf, then the same tree.  mean = (float)(sum / n): one rounding to float32.
 *   windows: the `len` entries from the oldest to the newest, sequentially, sums in float64; mean = sum / len in float64.
 *   max: op(a, b) = NaN if a or b is NaN, else a > b ? a : b;  min: ... a < b ? a : b.
 * Every workspace word that is read was written earlier in the same call: stale contents do not matter.
 *
 * Conventions as in rover_scaler.h: plain C, caller-owned DEVICE buffers, int return codes (ROVER_ERR_INVALID for a bad argument
 * or a workspace that is too small; the state is not touched then), rover_last_error() for the text, every call asynchronous on
 * `stream` and run on the device the state block lives on.  No allocation, no host synchronisation, no atomics.
 */
#ifndef ROVER_TRACKER_H
#define ROVER_TRACKER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ROVER_TRACKER_WINDOW     100    /* skrl: collections.deque(maxlen=100) */
#define ROVER_TRACKER_CHUNK      256    /* envs per workgroup of the step's first launch */
#define ROVER_TRACKER_MAX_SLOTS  4096
#define ROVER_TRACKER_HDR_WORDS  220    /* words in front of the slots */
#define ROVER_TRACKER_ACC_WORDS  20     /* words [0, 20): what a snapshot copies in front of the slots */

/* Bytes of a state block for n envs and `slots` user slots; 0 if n < 1 or slots outside [0, 4096]. */
size_t rover_tracker_state_bytes(int32_t n, int32_t slots);
/* Device workspace bytes of rover_tracker_step for n envs (20 bytes per chunk of 256 envs, rounded up to 8); 0 if n < 1. */
size_t rover_tracker_workspace_bytes(int32_t n);
/* 4-byte words rover_tracker_snapshot writes: 20 + 6 slots; 0 for slots outside [0, 4096]. */
size_t rover_tracker_snapshot_words(int32_t slots);

/* The initial state: everything zero, the maxima -inf, the minima +inf, n and slots in the header.  One launch. */
int rover_tracker_init(void *state, int32_t n, int32_t slots, void *stream);

/* One env step (see above).  rew: float32[n]; terminated, truncated: n flags of flag_bytes bytes each: 4 = float32, as the
 * collectors hold them (finished where terminated + truncated != 0), 1 = bool / uint8, as the envs return them (finished where
 * either is set); truncated may be NULL (nothing is truncated); ws: 8-byte aligned, at least rover_tracker_workspace_bytes(n).
 * Two launches: one workgroup per 256 envs (cum_r / cum_t, the chunk's count of finished envs by ballot and popcount per wave and
 * LDS across the waves, the chunk's max / min / sum), then one workgroup that
 * combines the chunk results, walks the chunks with finished envs in ascending order (each env's rank = the count of the chunks
 * before it + the waves before it + the lanes before it), writes the entries of rank >= K - 100 to ring slot (head + rank) mod
 * 100, zeroes cum_r / cum_t there, sets head = (head + K) mod 100, len = min(100, len + K) and folds the step into the
 * accumulators. */
int rover_tracker_step(void *state, int32_t n, int32_t slots, const float *rew, const void *terminated, const void *truncated,
                       int32_t flag_bytes, void *ws, size_t ws_bytes, void *stream);

/* Folds values[i] (DEVICE float32) into slot first_slot + i, i < count: sum (float64) += v, count += 1, max, min.  One launch.
 * ROVER_ERR_INVALID unless 0 <= first_slot, 1 <= count and first_slot + count <= slots. */
int rover_tracker_track(void *state, int32_t n, int32_t slots, int32_t first_slot, const float *values, int32_t count, void *stream);

/* Copies words [0, 20) and the slots (the layout above: sums, counts, maxima, minima) into out (DEVICE or host-mapped memory,
 * 8-byte aligned, rover_tracker_snapshot_words(slots) words), then clears the accumulators, the step counts and the slots; with
 * clear_window != 0 also head = len = 0.  cum_r and cum_t are kept.  One launch. */
int rover_tracker_snapshot(void *state, int32_t n, int32_t slots, void *out, int32_t clear_window, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_TRACKER_H */
