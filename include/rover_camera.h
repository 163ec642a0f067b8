/*
 * rover_camera.h -- C ABI of the rover's on-board depth camera (librover_hip.so).
 *
 * Replaces the depth half of the reference's camera env
 *     rover_envs/envs/navigation/entrypoints/rover_camera_env.py:18-76   RoverEnvCamera (camera prim + render products)
 *     rover_envs/envs/navigation/entrypoints/rover_camera_env.py:94-104  PytorchListenerRover.get_depth_data
 * The reference renders `distance_to_camera` with RTX.  The only geometry in its scene is the terrain mesh, which this library
 * already holds as the heightfield bound by rover_set_terrain (cells split along the (i, j) - (i+1, j+1) diagonal), so the depth
 * image is a ray cast against that triangle mesh.  RGB is not provided.
 *
 * Conventions as in rover_hip.h: plain C, caller-owned DEVICE buffers, int return codes, rover_last_error() for the text, all
 * calls asynchronous on `stream`.  The camera reads the state and terrain of a rover_sim handle; it has no handle of its own.
 */
#ifndef ROVER_CAMERA_H
#define ROVER_CAMERA_H

#include <stddef.h>
#include <stdint.h>

#include "rover_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pinhole camera rigidly mounted on the Body link.  Defaults = rover_camera_env.py:44-62. */
typedef struct rover_camera_config {
    int32_t width, height;          /* render product, pixels (:62: 160 x 90)                                          */
    float focal_length;             /* mm (:47: 2.12)                                                                   */
    float horizontal_aperture;      /* mm (:49: 6.055); f_x = width * focal_length / horizontal_aperture pixels         */
    float vertical_aperture;        /* mm; <= 0: square pixels (f_y = f_x, Isaac Sim's model; the default).  The stated
                                       2.968879962 (:50) would give f_y = height * focal_length / vertical_aperture      */
    float mount_pos[3];             /* m, in the Body frame (:55: -0.151, 0, 0.73428)                                   */
    float mount_quat[4];            /* (w, x, y, z) Body <- camera, USD camera convention: looks along -Z, up is +Y
                                       (:56: 0.64086, 0.29884, -0.29884, -0.64086; normalised by the library)           */
    float near_clip, far_clip;      /* m (:51: clippingRange (0.01, 1000000)); 0 <= near_clip < far_clip, far_clip may be
                                       +inf.  Every other float must be finite, or prepare / render return ROVER_ERR_INVALID */
} rover_camera_config;

/* The reference's camera prim attributes (rover_camera_env.py:44-56) and render-product size (:62). */
int rover_camera_default_config(rover_camera_config *cfg);
/* sizeof(rover_camera_config): lets a binding check its mirror of the struct. */
size_t rover_camera_config_bytes(void);

/* Bytes of the caller-owned device workspace the camera needs for the terrain bound to `sim` (a max-height pyramid over the
 * heightfield, about 1/64 of its size).  0 if no terrain is bound or `cfg` is invalid.  (The reference's RTX scene needs no
 * such structure from its caller: rover_camera_env.py:58-63 creates one render product per env.) */
size_t rover_camera_workspace_bytes(const struct rover_sim *sim, const rover_camera_config *cfg);

/* Build the max-height pyramid of the terrain currently bound to `sim` into `ws` (`bytes` >= rover_camera_workspace_bytes).
 * Call again after every rover_set_terrain* on `sim`.  Replaces the scene set-up of rover_camera_env.py:58-71.
 * rover_lidar_prepare (rover_lidar.h) builds the same pyramid and writes the same record in the handle: one prepared workspace
 * serves rover_camera_render and rover_lidar_cast alike, whichever call prepared it, and the last prepare wins. */
int rover_camera_prepare(struct rover_sim *sim, const rover_camera_config *cfg, void *ws, size_t bytes, void *stream);

/* depth (num_envs, height, width) fp32, row-major: Euclidean distance from the optical centre to the first hit of each pixel's
 * ray (through the pixel centre) with the terrain's triangle mesh, for the pose the state of `sim` holds; +inf where the ray
 * leaves the terrain, climbs above its highest point or passes the far clip; hits nearer than the near clip do not count.
 * Replaces `distance_to_camera` as PytorchListenerRover.get_depth_data returns it (rover_camera_env.py:100-104) before its
 * permute(0, 2, 1).  ROVER_ERR_STATE: no terrain or state bound, terrain re-bound since rover_camera_prepare (or `ws` is not
 * the prepared workspace), or called between rover_step_begin and rover_step_finish. */
int rover_camera_render(struct rover_sim *sim, const rover_camera_config *cfg, const void *ws, float *depth, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ROVER_CAMERA_H */
