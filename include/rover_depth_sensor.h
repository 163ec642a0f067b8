/*
 * rover_depth_sensor.h -- C ABI of the depth camera's sensor model as one launch (librover_hip.so).
 *
 * rover_camera_render gives the exact range along each pixel's ray.  A stereo or structured-light camera does not: its error grows
 * with the square of the range, its depth comes in steps (disparity is quantised), it has a working range outside which it reports
 * "no data", and it loses pixels, mostly along occlusion edges.  rover_depth_sensor_apply puts these four effects on `n` row-major
 * images of height x width floats.  Per pixel, with z the rendered depth, each arithmetic step one fp32 operation rounded once (no
 * contraction), in this order:
 *   1 range     valid = (z >= range_min) && (z <= range_max): a NaN, a +inf miss and a negative value are invalid.  An invalid pixel
 *               skips to step 6.
 *   2 edge      over the 4-neighbours INSIDE the image, in the order up, down, left, right (the left neighbour of column 0 and the
 *               right neighbour of the last column do not exist: the flat index does not wrap into the next row), with zn the
 *               neighbour's RENDERED depth: a neighbour that is invalid by step 1 makes the pixel an edge when edge_at_invalid != 0;
 *               any other makes it one when fabsf(z - zn) > edge_rel * fminf(z, zn).
 *   3 dropout   p = edge ? p_edge : p_drop; the pixel becomes invalid when u < p, u the pixel's uniform in (0, 1): p = 0 never
 *               drops, p = 1 always does.
 *   4 noise     t = z * sigma2; t = t + sigma1; t = z * t; s = t + sigma0; m = s * e; z = z + m, e the pixel's standard normal:
 *               sigma(z) = sigma0 + sigma1 z + sigma2 z^2.
 *   5 disparity only when disparity_step > 0: d = fb / z; k = rintf(d * inv_step) (ties to even); the pixel is invalid if
 *               !(k >= 1); otherwise z = fb / (k * disparity_step).  Both divisions are correctly rounded.  fb is the focal length
 *               in pixels times the baseline in metres, inv_step the caller's fp32 of 1 / disparity_step.
 *   6 fill      an invalid pixel is written as invalid_value.
 *
 * The draws are counter-based and addressed by ABSOLUTE pixel p = i * width + j: Philox4x32-10 keyed by (seed lo, seed hi), the
 * counter of the four pixels 4 q .. 4 q + 3 ("quad" q) of image r is
 *     (lo32(env_id_offset + r), lo32(counter), hi32(counter), tag | q)
 * exactly as in rover_obs_post.h, under two tags of this header's own:
 *     ROVER_DEPTH_SENSOR_STREAM_NORMAL    words (0, 1) give pixels 4 q (cosine branch) and 4 q + 1 (sine branch) by Box-Muller,
 *                                         words (2, 3) give 4 q + 2 and 4 q + 3 (rover_obs_post.h's gaussian mapping)
 *     ROVER_DEPTH_SENSOR_STREAM_DROPOUT   pixel p takes word p % 4: u = ((w >> 9) + 0.5) * 2^-23
 * Neither shares its high half with another draw of this library; the low 16 bits carry the quad, so height * width <=
 * ROVER_DEPTH_SENSOR_MAX_PIXELS = 16384 (which also lets one image sit in LDS).  The draws do not depend on the launch geometry or on
 * how the envs are split over ranks.  There is no state: the caller's (seed, env_id_offset, counter) is the checkpoint.
 *
 * Conventions as in rover_obs_post.h: plain C, caller-owned DEVICE buffers, int return codes, rover_last_error() for the text,
 * asynchronous on `stream` and run on the device `dst` lives on.  One launch; no workspace, no allocation, no host synchronisation,
 * no float atomics.  The arguments are checked before the device is looked at, so every refusal below also works on a host without
 * a GPU.
 */
#ifndef ROVER_DEPTH_SENSOR_H
#define ROVER_DEPTH_SENSOR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ROVER_DEPTH_SENSOR_MAX_PIXELS 16384        /* 4096 quads; one image is at most 64 KB of LDS */

/* the streams' names in the high half of counter word 3 */
#define ROVER_DEPTH_SENSOR_STREAM_NORMAL  0x444E0000u    /* "DN": the axial noise's normals */
#define ROVER_DEPTH_SENSOR_STREAM_DROPOUT 0x44550000u    /* "DU": the dropout's uniforms    */

typedef struct rover_depth_sensor_cfg {
    float range_min, range_max;          /* metres; range_max may be +inf                                         */
    float sigma0, sigma1, sigma2;        /* sigma(z) = sigma0 + sigma1 z + sigma2 z^2, each >= 0                   */
    float p_drop, p_edge;                /* dropout probability off / on an edge, in [0, 1]                       */
    float edge_rel;                      /* relative depth step that makes an edge, >= 0                          */
    int32_t edge_at_invalid;             /* != 0: a neighbour outside the range makes an edge                     */
    float disparity_step;                /* pixels; 0: no quantisation, fb and inv_step are not read              */
    float fb;                            /* focal length [px] * baseline [m]                                      */
    float inv_step;                      /* fp32 of 1 / disparity_step                                            */
    float invalid_value;                 /* what an invalid pixel reads; not NaN                                  */
} rover_depth_sensor_cfg;

size_t rover_depth_sensor_cfg_bytes(void);

/* dst[r * pitch_floats + p] = sensor(src[r * pitch_floats + ...]), r < n, p < height * width; one launch.
 *   cfg            HOST struct; it is copied before the call returns.
 *   src, dst       device floats, 4-byte aligned: an image may start at any 4-byte offset (16-byte accesses where the offset allows,
 *                  the values are the same either way).  dst may equal src; for each image the result is as if all of src had been
 *                  read before any of dst is written.  Any other overlap of the two is refused.  Floats between two images (the
 *                  pitch's gap) are neither read nor written.
 *   height, width  of one image; pitch_floats >= height * width is the distance between two images.
 *   valid_out      NULL, or n int32 on the device: the pixels of each image that leave the kernel valid (an integer reduction: it
 *                  does not depend on order).
 *   seed, env_id_offset, counter      the draw address (above).
 * ROVER_ERR_UNSUPPORTED, and nothing launched, for height * width > ROVER_DEPTH_SENSOR_MAX_PIXELS.
 * ROVER_ERR_INVALID, and nothing launched, for: a NULL cfg, src or dst; n <= 0; height <= 0 or width <= 0; pitch_floats <
 * height * width; src, dst or valid_out not 4-byte aligned; src and dst overlapping without being equal; a non-finite or negative
 * sigma0, sigma1, sigma2 or edge_rel; p_drop or p_edge outside [0, 1] or NaN; range_min NaN or negative; range_max NaN or <
 * range_min; disparity_step negative or not finite; with disparity_step > 0, an fb or inv_step that is not finite and positive;
 * invalid_value NaN. */
int rover_depth_sensor_apply(const rover_depth_sensor_cfg *cfg, const float *src, float *dst, int32_t height, int32_t width,
                             int64_t pitch_floats, int32_t n, uint64_t seed, uint64_t env_id_offset, uint64_t counter,
                             int32_t *valid_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_DEPTH_SENSOR_H */
