/*
 * rover_dagger_conv.h -- C ABI of the fused DAgger distillation into a student that reads the camera the reference defines: the
 * 160 x 90 depth image of RoverEnvCamera through a small learned convolutional stem (librover_hip.so).
 *
 * rover_dagger.h reached a trainer by shrinking the camera to 31 x 31, where the image is the 961-wide scan input itself.  Here the
 * image keeps its native size and a stem turns it into the 961 feature columns of the 965-wide student row; the reference network
 * behind it (rover_policy_default_desc(d, 2, 1)), the teacher, the label, the Philox mixing draw, rover_dagger_act, the replay
 * memory, the loss head and clip / Adam / replicas are rover_dagger.h's, unchanged.  Per image, with d the row-major (90, 160)
 * render buffer of rover_camera_render at the default camera:
 *
 *     x(r, s)    = depth_scale * min(d(r, s), depth_clip);  d = depth_clip where the pixel is NaN, +-inf or negative    (as rover_dagger.h)
 *     pre_c(i,j) = b1[c] + sum_{u < 6, v < 10} W1[c][u][v] * x(3 i - 3 + u, 5 j + v)      c < 8, i < 31, j < 31; x = 0 outside rows [0, 90)
 *     h_c        = pre_c > 0 ? pre_c : 0.01 * pre_c
 *     y(i, j)    = b2 + sum_c w2[c] * h_c(i, j)
 *     row[4 + 31 i + j] = y(i, j);   row[0:4] = nan_to_num(env_row[0:4], nan = 0, posinf = FLT_MAX, neginf = 0)
 *
 * i.e. Conv2d(1 -> 8, kernel (6, 10), stride (3, 5), padding (3, 0)), LeakyReLU(0.01), Conv2d(8 -> 1, kernel 1).  Adjacent windows
 * overlap by half in both directions; output rows 0 and 30 read three padded rows each.  The stem's parameters are
 * ROVER_DAGGER_CONV_STEM_FLOATS = 497 floats packed as W1[8][6][10], b1[8], w2[8], b2.  The reference's slicing quirk carries
 * over (models.py:95): the encoder reads columns [3, 964), so feature (30, 30) is computed, stored and never read, and its
 * gradient is exactly 0.  The derivative of the LeakyReLU at a pre-activation of exactly 0 is the slope (torch's x > 0 ? 1 : slope).
 *
 * Parameter vector (params, grad, adam_m, adam_v alike): [ head | stem ]: the head is rover_dagger.h's vector
 * (rover_dagger_param_floats floats), the stem's 497 floats follow at rover_dagger_conv_stem_offset, padded with zeros to 512.
 *
 * Image ring: (image_slots, num_envs, 14400) floats of x (preprocessed pixels, not metres), addressed by the replay memory's own
 * ring row number slot * num_envs + env; it needs at least as many slots as the observation ring.  The ring slot's feature columns
 * hold the stem's output under the parameters of the step that wrote them (what rover_dagger_act's student reads); the update
 * recomputes them from the image ring under the current parameters.
 *
 * Numerics (bit-reproducible from run to run; every order a function of n alone; no float atomics):
 *   - ONE device function forms a feature from the x image and the parameters, in every kernel of every launch, so the collector's
 *     features, the update's features and the backward's recomputed pre-activations agree on the bits (the torch specification is
 *     compared under a tolerance).  Its order: acc_c = 0; for u = 0 .. 5, for v = 0 .. 9: acc_c = fma(W1[c][u][v], x, acc_c) (a padded
 *     tap multiplies a stored zero); pre_c = acc_c + b1[c]; y = b2; for c = 0 .. 7: y = fma(w2[c], h_c, y).
 *   - stem backward, per sampled row r and output o = 31 i + j with g = dRow[r][4 + o]:
 *         db2 += g;  dw2[c] += g * h_c;  dpre_c = (g * w2[c]) * (pre_c > 0 ? 1 : 0.01);  db1[c] += dpre_c;
 *         dW1[c][u][v] += dpre_c * x(3 i - 3 + u, 5 j + v)
 *     Rows are cut into fixed chunks of rover_dagger_conv_chunk_rows() = 8, one 512-thread workgroup each.  Inside a chunk: lane
 *     l of wave w owns outputs 128 w + l and 128 w + 64 + l of every row and adds its db2 / dw2 / db1 terms in (row, output)
 *     order, the 512 threads' sums go through a fixed halving tree; dW1 is an MFMA (v_mfma_f32_16x16x4_f32) chain per wave over
 *     the rows of the chunk in order and, inside a row, over the wave's 128 outputs in ascending groups of 4, the eight waves'
 *     sums are added in wave order.  The chunk partials are added in chunk order (rover_td3.h's combine kernel).
 *   - the input gradient dRow[:, 4 + p] = sum_j dZ1[:, j] W_enc1[j][1 + p], p < 960, is rover_td3.h's backward kernel without an
 *     activation derivative; column 964 (and 0 .. 3, which nothing learns from) is written as 0.
 *   - everything else (gather, dense layers, loss head, gradient norm, clip, Adam, replicas) as rover_dagger.h states it; the norm
 *     is taken over the whole vector [head | stem], as clip_grad_norm_ over both parameter lists computes it.
 *
 * Conventions as in rover_dagger.h: plain C, caller-owned DEVICE buffers, int return codes, rover_last_error(), every call
 * asynchronous on `stream`, no allocation, no host synchronisation; bad arguments are refused without a launch.
 */
#ifndef ROVER_DAGGER_CONV_H
#define ROVER_DAGGER_CONV_H

#include <stddef.h>
#include <stdint.h>

#include "rover_dagger.h"
#include "rover_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ROVER_DAGGER_CONV_IMG_H 90
#define ROVER_DAGGER_CONV_IMG_W 160
#define ROVER_DAGGER_CONV_PIXELS 14400
#define ROVER_DAGGER_CONV_STEM_FLOATS 497

/* 497 */
size_t rover_dagger_conv_stem_floats(void);
/* Floats of the vector [head | stem | padding]; 0 if `student` is not rover_policy_default_desc(2, 1) packed by rover_policy_pack. */
size_t rover_dagger_conv_param_floats(const rover_policy_desc *student);
/* First float of the stem inside that vector (rover_dagger_param_floats(student)); 0 under the same condition. */
size_t rover_dagger_conv_stem_offset(const rover_policy_desc *student);
/* Rows per chunk of the stem backward's reduction (8). */
int32_t rover_dagger_conv_chunk_rows(void);
/* Device workspace bytes of rover_dagger_conv_update over up to `max_rows` sampled rows; 0 if max_rows < 1. */
size_t rover_dagger_conv_workspace_bytes(int32_t max_rows);

/* One launch, one 512-thread workgroup per env: rover_dagger_record for this student (with rew .. idx_out NULL: rover_dagger_rows).
 *   stem             (497)          the stem's current parameters
 *   depth            (n, 14400)     the render buffer, row-major (90, 160); img_h, img_w must be 90, 160
 *   env_raw          (n, 965)       the env's raw observation rows
 *   ring_slot_out    (n, 965)       columns 0 .. 3 sanitised, columns 4 .. 964 the stem's features
 *   image_slot_out   (n, 14400)     x, the preprocessed image (the image ring's slot)
 *   teacher_rows_out (n, 965)       nan_to_num(env_raw); may be NULL
 * and rover_dagger_record's bookkeeping, argument for argument (rew, terminated, rew_out, term_out all or none NULL; ring_pos_entry
 * and idx_out may be NULL; mem_rows in [1, 2^32] when indices are asked for; the same index stream and tag).  depth and
 * image_slot_out must be 16-byte aligned; the outputs must not alias the inputs. */
int rover_dagger_conv_rows(const rover_dagger_hparams *h, const float *stem, const float *depth, int32_t img_h, int32_t img_w,
                           const float *env_raw, int32_t n, float *ring_slot_out, float *image_slot_out, float *teacher_rows_out,
                           const float *rew, const uint8_t *terminated, float *rew_out, uint8_t *term_out, int32_t *ring_pos_entry,
                           int32_t ring_pos_value, int64_t *idx_out, int32_t batch, int64_t mem_rows, uint64_t counter, void *stream);

/* One imitation step over n sampled rows, rover_dagger_update with the stem in front: gather, the stem's forward over the sampled
 * rows' images under the current parameters (into a gathered copy of the rows), six dense layers, the loss head, five backward
 * layers, the input gradient, the stem's backward, the weight gradients, ONE gradient norm over head and stem, Adam on both and the
 * head's n_copies replicas (22 launches).  An index outside [0, valid_rows) or a ring position outside [0, slots) reads row 0 of
 * both rings instead and sets bad_index.
 *   params, grad, adam_m, adam_v   rover_dagger_conv_param_floats floats each, 16-byte aligned
 *   image_ring                     (image_slots, num_envs, 14400), 16-byte aligned; image_slots >= slots; img_h, img_w must be 90, 160
 *   dz_out   (n, 2)     dz of the head; may be NULL
 *   rows_out (n, 965)   the gathered rows with the recomputed features; may be NULL
 *   drow_out (n, 965)   dL/drow: columns 4 .. 963 the input gradient, the others 0; may be NULL
 * ws: rover_dagger_conv_workspace_bytes(n) bytes or more, 16-byte aligned.  state: a rover_dagger_state. */
int rover_dagger_conv_update(const rover_policy_desc *student, const rover_dagger_hparams *h, float *params, float *grad,
                             float *adam_m, float *adam_v, const float *obs_ring, const float *image_ring, int32_t image_slots,
                             int32_t img_h, int32_t img_w, int32_t slots, int32_t num_envs, const int32_t *ring_pos,
                             const float *labels, const int64_t *idx, int32_t n, int64_t valid_rows, void *ws, size_t ws_bytes,
                             void *state, float *replicas, int32_t n_copies, float *dz_out, float *rows_out, float *drow_out,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_DAGGER_CONV_H */
