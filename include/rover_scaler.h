/*
 * rover_scaler.h -- C ABI of skrl's RunningStandardScaler at any width up to 1024 (librover_hip.so).
 *
 * The reference's agent files (rover_ppo.yaml, rover_rpo.yaml, rover_trpo.yaml: state_preprocessor / value_preprocessor, turned
 * into skrl.resources.preprocessors.torch.RunningStandardScaler by rover_envs/utils/config.py:76-96) standardise the 965-wide
 * observation rows and the 1-wide values.  rover_lift_train.h has the same scaler for the lift task, capped at 64 columns and
 * one workgroup per column; these entries are width-generic and split the rows over workgroups.
 *
 * Scaler block (device memory, 8-byte aligned, rover_scaler_doubles(width) doubles), the layout of rover_lift_train.h:
 *     double mean[width], var[width], count;     initial state mean 0, var 1, count 1 (the caller writes it)
 *   train:    batch mean m_b and unbiased variance v_b per column in float64 (two passes over the rows: the mean, then the sum
 *             of squared deviations from it), count c_b = rows; then skrl's _parallel_variance:
 *             delta = m_b - mean; tot = count + c_b;
 *             var = (var * count + v_b * c_b + delta^2 * count * c_b / tot) / tot;  mean = mean + delta * c_b / tot;  count = tot
 *   forward:  clamp((x - (float)mean) / (sqrtf((float)var) + eps), -clip, clip)          (fp32, no contraction)
 *   inverse:  sqrtf((float)var) * clamp(x, -clip, clip) + (float)mean                    (fp32, a product then a sum)
 * clamp propagates NaN, as torch.clamp does.
 *
 * Conventions as in rover_train.h: plain C, caller-owned DEVICE buffers, int return codes (ROVER_ERR_INVALID for a bad argument
 * or a workspace that is too small), rover_last_error() for the text, every call asynchronous on `stream` and run on the device
 * the scaler block lives on.  No allocation, no host synchronisation, no atomics.
 *
 * Reduction order of rover_scaler_train (a function of `rows` alone, so every result is bit-reproducible from run to run whatever
 * the order the workgroups run in; the only synchronisation between workgroups is the boundary between two launches):
 *   1. the rows are cut into chunks of 64 (chunk k = rows [64 k, 64 k + 64) of idx, the last one ragged).  One 256-thread
 *      workgroup per (chunk, block of 64 columns): lane l of wave q owns column 64 b + l and adds the chunk's rows q, q + 4,
 *      q + 8, ... in ascending order in float64; the four wave partials combine as (p0 + p1) + (p2 + p3) into the workspace;
 *   2. one thread per column adds the chunk sums in ascending chunk order and divides by rows: the batch mean;
 *   3. as 1. with (x - mean)^2 in place of x;
 *   4. one thread per column adds the chunk sums in ascending chunk order, divides by rows - 1 and merges as above.
 * Every workspace word that is read was written earlier in the same call: stale contents do not matter.
 */
#ifndef ROVER_SCALER_H
#define ROVER_SCALER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ROVER_SCALER_MAX_WIDTH 1024

typedef struct rover_scaler_hparams {
    float eps;     /* RunningStandardScaler epsilon (1e-8)      */
    float clip;    /* RunningStandardScaler clip_threshold (5)  */
} rover_scaler_hparams;

/* flags of rover_scaler_apply */
#define ROVER_SCALER_INVERSE  1   /* the inverse transform instead of the forward one */
#define ROVER_SCALER_SANITISE 2   /* first x = nan_to_num(x, nan = 0, posinf = FLT_MAX, neginf = 0), the rollout collector's (rover_rollout.h) */

/* eps 1e-8, clip 5 */
int    rover_scaler_default_hparams(rover_scaler_hparams *h);
size_t rover_scaler_hparams_bytes(void);

/* Doubles of a scaler block of `width` columns (2 width + 1); 0 if width < 1 or width > 1024. */
size_t rover_scaler_doubles(int32_t width);
/* Device workspace bytes of rover_scaler_train for up to `max_rows` rows of `width` columns; 0 for a width outside [1, 1024] or
 * max_rows < 2. */
size_t rover_scaler_workspace_bytes(int32_t width, int32_t max_rows);

/* Updates the block with the rows idx[0 .. rows) of x (B, width) fp32 row-major; idx: int64 DEVICE indices in any order, a
 * repeated index counts as one more row; idx == NULL: rows 0 .. rows.  rows >= 2 (the unbiased variance of one row is NaN in
 * torch; ROVER_ERR_INVALID here, as in rover_lift_ppo_standardize).  `h` is not read by the statistics; it is checked for NULL
 * only.  Four launches (see the reduction order above). */
int rover_scaler_train(const rover_scaler_hparams *h, double *scaler, int32_t width, const float *x, const int64_t *idx,
                       int32_t rows, void *ws, size_t ws_bytes, void *stream);

/* rover_scaler_train behind a gate word (device memory, 4-byte aligned; rover_ppo_epoch.stop of rover_train_gate.h): each of the
 * four launches returns at once when *gate != 0 and the block and the workspace are untouched; otherwise bit-identical to
 * rover_scaler_train.  No kernel of this header writes the gate.  skrl standardises (and in the first epoch trains) a minibatch's
 * states before it computes the KL, so the minibatch that stops an epoch still trains the state scaler and the skipped ones do
 * not: the gate is read as the minibatch before left it. */
int rover_scaler_train_gated(const rover_scaler_hparams *h, double *scaler, int32_t width, const float *x, const int64_t *idx,
                             int32_t rows, void *ws, size_t ws_bytes, const int32_t *gate, void *stream);

/* out = scaler(x), one launch, no update of the block.
 *   idx == NULL: rows [0, rows) of x into rows [0, rows) of out.
 *   idx given:   row idx[i] of x into row idx[i] of out, i < rows: in place within a (B, width) image, rows not named are not
 *                touched.  A repeated index is written twice with the same value; with out == x the indices must be distinct.
 *   flags:       ROVER_SCALER_INVERSE, ROVER_SCALER_SANITISE (see above), or both (sanitise first).
 *   raw_out:     may be NULL; otherwise it receives the input rows as they enter the transform (sanitised when the flag is set)
 *                at the same row positions as `out`: the rollout buffer's slot, filled by the same pass.
 * out may alias x exactly (out == x); raw_out must not be x or out (ROVER_ERR_INVALID).  x, out and raw_out are 4-byte aligned
 * float arrays of pitch `width`: rows start at any 4-byte offset.  Where x, out and raw_out share their offset from 16-byte
 * alignment a row is moved as a scalar head up to the next 16-byte boundary, 16-byte vectors and a scalar tail; otherwise
 * element by element.  The values do not depend on which. */
int rover_scaler_apply(const rover_scaler_hparams *h, const double *scaler, int32_t width, const float *x, const int64_t *idx,
                       int32_t rows, int32_t flags, float *out, float *raw_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_SCALER_H */
