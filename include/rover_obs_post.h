/*
 * rover_obs_post.h -- C ABI of ORBIT's observation post-processing (noise -> clip -> scale) as one launch (librover_hip.so).
 *
 * The reference switches observation corruption on (rover_env_cfg.py ObservationCfg.PolicyCfg.__post_init__: enable_corruption =
 * True) and imports ORBIT's additive uniform noise for it (rover_env_cfg.py:23, Unoise).  ORBIT's ObservationManager.compute_group
 * finishes a term as value -> + noise -> clip -> * scale.  rover_obs_post_apply does that in place on `n` rows of `width` floats, for
 * up to ROVER_OBS_POST_MAX_SEGMENTS column ranges of the row, each with its own noise, clip and scale; the same entry corrupts a
 * depth image (one row = one image, row-major).
 *
 * Per element of a segment, each operation one fp32 operation rounded once (no contraction), in this order:
 *     uniform   x = (x + u * b) + a          a = n_min, b = span = (float)((double)n_max - (double)n_min), u in (0, 1)
 *     gaussian  x = (x + a) + b * e          a = mean, b = std, e a standard normal
 *     constant  x = x + a                    a = bias
 *     clip      x = clamp(x, clip_lo, clip_hi) as torch.clip: a NaN stays a NaN, -inf goes to clip_lo, +inf to clip_hi.  A clip
 *               treats -0 < +0: clamp(x) = min(max(x, clip_lo), clip_hi) under that order (IEEE 754-2019 maximum / minimum), so
 *               clamp(+0, lo = -0) = +0, clamp(-0, lo = +0) = +0 and clamp(+0, hi = -0) = -0, whatever the operand order.
 *     scale     x = x * scale                only when scale != 1
 * Columns outside every segment are neither read nor written.
 *
 * The draws are counter-based and addressed by ABSOLUTE column: they do not depend on how the row is cut into segments, on the
 * launch geometry, or on how the rows are split over ranks.  Philox4x32-10 keyed by (seed lo, seed hi); the counter of the four
 * columns 4 q .. 4 q + 3 ("quad" q) of row r is
 *     (lo32(env_id_offset + r), lo32(counter), hi32(counter), tag | q)
 * with q in the low 16 bits of word 3 and `tag` in the high 16: width <= ROVER_OBS_POST_MAX_WIDTH = 262144.
 *     uniform   column c takes word c % 4: u = ((w >> 9) + 0.5) * 2^-23
 *     gaussian  words (0, 1) give columns 4 q (cosine branch) and 4 q + 1 (sine branch) by Box-Muller, words (2, 3) give
 *               4 q + 2 and 4 q + 3: rho = sqrtf(-2 logf(u(w_a))), (e_cos, e_sin) = rho * sincospif(2 u(w_b))
 * Tags: ROVER_OBS_POST_STREAM_ROW for observation rows, ROVER_OBS_POST_STREAM_DEPTH for depth images (and rover_lidar.h's
 * ROVER_LIDAR_STREAM_NOISE for lidar frames); none shares its high half with another draw of this library.  There is no state: the caller's (seed, env_id_offset, counter) is the checkpoint.
 *
 * Conventions as in rover_scaler.h: plain C, caller-owned DEVICE buffers, int return codes (ROVER_ERR_INVALID for a bad argument,
 * with no launch), rover_last_error() for the text, asynchronous on `stream` and run on the device `rows` lives on.  No
 * allocation, no host synchronisation, no atomics.  The arguments are checked before the device is looked at, so every refusal
 * below also works on a host without a GPU.
 */
#ifndef ROVER_OBS_POST_H
#define ROVER_OBS_POST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ROVER_OBS_POST_MAX_SEGMENTS 8
#define ROVER_OBS_POST_MAX_WIDTH    262144      /* 65536 quads: the quad index is the low half of Philox counter word 3 */

#define ROVER_OBS_POST_NOISE_NONE     0
#define ROVER_OBS_POST_NOISE_UNIFORM  1
#define ROVER_OBS_POST_NOISE_GAUSSIAN 2
#define ROVER_OBS_POST_NOISE_CONSTANT 3

/* the `tag` argument: the stream's name in the high half of counter word 3 */
#define ROVER_OBS_POST_STREAM_ROW   0x4F500000u    /* "OP": observation rows */
#define ROVER_OBS_POST_STREAM_DEPTH 0x4F440000u    /* "OD": depth images     */

typedef struct rover_obs_post_segment {
    int32_t col_lo, col_hi;       /* the columns [col_lo, col_hi) of the row                                  */
    int32_t noise;                /* ROVER_OBS_POST_NOISE_*                                                   */
    float a, b;                   /* uniform: n_min, span; gaussian: mean, std; constant: bias, unused       */
    int32_t has_clip;             /* 0: no clip, clip_lo / clip_hi are not read                              */
    float clip_lo, clip_hi;
    float scale;                  /* 1: no multiplication                                                    */
} rover_obs_post_segment;

size_t rover_obs_post_segment_bytes(void);

/* Post-processes rows[r * pitch_floats + c], r < n, c in a segment, in place; one launch.
 *   seg, n_seg     HOST array of 1 .. ROVER_OBS_POST_MAX_SEGMENTS segments, in any order; it is copied before the call returns.
 *   rows           device floats, 4-byte aligned: a row may start at any 4-byte offset.  Where a row's offset allows, a quad moves as
 *                  one 16-byte access, otherwise element by element; the values are the same either way.
 *   width, pitch   columns of a row and the distance between two rows in floats, pitch_floats >= width.
 *   seed, env_id_offset, counter, tag     the draw address (above); `tag` has its low 16 bits clear.
 * ROVER_ERR_INVALID, and nothing launched, for: a NULL seg or rows; n <= 0; width <= 0 or > ROVER_OBS_POST_MAX_WIDTH;
 * pitch_floats < width; n_seg outside 1 .. 8; a segment that is empty (col_lo >= col_hi), leaves the row (col_lo < 0 or
 * col_hi > width) or overlaps another; an unknown noise kind; a non-finite a, b, scale or (with has_clip) clip bound; span < 0;
 * std < 0; clip_lo > clip_hi; a tag with any of its low 16 bits set; rows not 4-byte aligned. */
int rover_obs_post_apply(const rover_obs_post_segment *seg, int32_t n_seg, float *rows, int32_t width, int64_t pitch_floats,
                         int32_t n, uint64_t seed, uint64_t env_id_offset, uint64_t counter, uint32_t tag, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_OBS_POST_H */
