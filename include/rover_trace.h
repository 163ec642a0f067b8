/*
 * rover_trace.h -- C ABI of the device-side episode recorder (librover_hip.so).
 *
 * Replaces, per env step of a data-collection loop, what isaac_rover_orbit_amd/trace.py: EpisodeRecorder.append_to_buffer does on the
 * host (the reference's DataRecorderBase.append_to_buffer, rover_envs/utils/recorder/data_recorder/base.py): one row of every
 * dataset joins its env's open episode, and the episodes of the envs that are done are emitted, whole and contiguous, in
 * (step of completion, env id) order.  Here the rows stay on the device until a drain:
 *
 *     per step   rover_trace_append      TWO launches, nothing read back, nothing written from the host:
 *                  append kernel         stage[s][e][(head[e] + len[e]) % R] = row e of stream s, for every stream and env
 *                  commit kernel         one workgroup, envs in id order: len[e] += 1; for a done env one descriptor
 *                                        (env, start, len, offset) joins the list, offset = the running row total, and
 *                                        head[e] = (start + len) % R, len[e] = 0, pending[e] += len
 *     at close   rover_trace_commit_all  the commit kernel with "every env with len > 0 is done" and no row added
 *     per drain  rover_trace_gather      output row r of the concatenated episodes, r in [r0, r0 + rows): binary search of its
 *                                        descriptor on `offset`, then out[s][r - r0] = stage[s][env][(start + r - offset) % R]
 *                rover_trace_drained     empties the descriptor list (count, row total, pending[])
 *
 * A stream is a sequence of opaque byte rows: row_bytes bytes per env and step, copied as they come (NaN payloads, -0.0 and
 * infinities included).  The one exception is ROVER_TRACE_BOOL, which stores byte != 0 (numpy's astype(bool) of a done flag).
 * Rows move in 16-byte pieces where the source and the destination row both allow it, in 4-byte or 1-byte pieces otherwise;
 * a source row may be only 4-byte aligned (an observation row is 3860 bytes) or have an odd width.
 *
 * The state block (rover_trace_state_bytes, int32 words): words 0 .. 15 are the header
 *     [0] episodes in the descriptor list   [1] sticky status (ROVER_TRACE_ST_*)   [2] rows in the descriptor list
 * then head[n], len[n], pending[n], and from word 16 + 4 * ceil(3 n / 4) on desc_cap descriptors of four words
 * (env, start, len, offset).  The block must be 16-byte aligned.
 *
 * Bounds.  Every staged row lands at slot (head + len) % R of its own env's ring, so no call writes outside the stage buffers
 * whatever the state holds.  A row that would make an episode longer than max_episode_rows, or that would overwrite a row that
 * is not drained yet (pending + len = R), is NOT staged: the status word takes ROVER_TRACE_ST_EPISODE / ROVER_TRACE_ST_RING and
 * stays set.  A descriptor beyond desc_cap is not written either (ROVER_TRACE_ST_DESC).  With a drain at least every D steps
 * and R >= max_episode_rows + D none of the three can happen while episodes keep to max_episode_rows.
 *
 * Conventions as in rover_td3_collect.h: plain C, caller-owned device buffers, int return codes, rover_last_error(), asynchronous
 * on `stream`, no allocation, no host synchronisation.  Bad arguments return ROVER_ERR_INVALID without a launch.
 */
#ifndef ROVER_TRACE_H
#define ROVER_TRACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ROVER_TRACE_MAX_STREAMS 16
#define ROVER_TRACE_HEADER_WORDS 16
#define ROVER_TRACE_COMMIT_CHUNK 256   /* envs the commit kernel visits per pass (its workgroup size) */

#define ROVER_TRACE_BOOL 1             /* stream flag: store byte != 0; row_bytes <= 16 only */

#define ROVER_TRACE_ST_EPISODE 1       /* an episode would have exceeded max_episode_rows */
#define ROVER_TRACE_ST_RING    2       /* a ring would have overwritten rows that are not drained */
#define ROVER_TRACE_ST_DESC    4       /* the descriptor list was full */

typedef struct rover_trace_stream {
    const void *src;        /* append: row e at src + e * src_pitch; unused by gather */
    int64_t     src_pitch;  /* bytes, >= row_bytes */
    void       *stage;      /* row (e, slot) at stage + (e * R + slot) * stage_pitch */
    int64_t     stage_pitch;/* bytes, >= row_bytes (rover_trace_stage_pitch pads to 16- or 4-byte multiples) */
    void       *out;        /* gather: output row i at out + i * out_pitch; unused by append */
    int64_t     out_pitch;  /* bytes, >= row_bytes */
    int32_t     row_bytes;  /* > 0 */
    int32_t     flags;      /* 0 or ROVER_TRACE_BOOL */
} rover_trace_stream;

size_t rover_trace_stream_bytes(void);                       /* sizeof(rover_trace_stream) */

/* staging pitch of a row: row_bytes rounded up to 16 (rows of 16 bytes or more) or to 4; 0 for row_bytes <= 0 */
size_t rover_trace_stage_pitch(int32_t row_bytes);
/* n * R * rover_trace_stage_pitch(row_bytes); 0 on bad arguments */
size_t rover_trace_stage_bytes(int32_t n, int32_t R, int32_t row_bytes);
/* bytes of the state block; 0 on bad arguments (n <= 0, desc_cap <= 0) */
size_t rover_trace_state_bytes(int32_t n, int32_t desc_cap);

/* zeroes the state block (one launch) */
int rover_trace_init(int32_t *state, int32_t n, int32_t desc_cap, void *stream);

/* One env step: the append launch over `streams`, then the commit launch over done[0 .. n) (one byte per env, != 0: done).
 * Requires 1 <= n_streams <= ROVER_TRACE_MAX_STREAMS, max_episode_rows >= 1, R >= max_episode_rows + 1, n * R < 2^31. */
int rover_trace_append(const rover_trace_stream *streams, int32_t n_streams, int32_t *state, int32_t n, int32_t R,
                       int32_t max_episode_rows, int32_t desc_cap, const uint8_t *done, void *stream);

/* the commit launch alone, every env with len > 0 counting as done (close) */
int rover_trace_commit_all(int32_t *state, int32_t n, int32_t R, int32_t desc_cap, void *stream);

/* One launch: output rows [r0, r0 + rows) of the concatenated committed episodes into every stream's `out`.  Rows at or beyond the
 * state's row total are left untouched. */
int rover_trace_gather(const rover_trace_stream *streams, int32_t n_streams, const int32_t *state, int32_t n, int32_t R,
                       int32_t desc_cap, int32_t r0, int32_t rows, void *stream);

/* after a drain: count = 0, rows = 0, pending[] = 0; head[], len[] and the status stay (one launch) */
int rover_trace_drained(int32_t *state, int32_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_TRACE_H */
