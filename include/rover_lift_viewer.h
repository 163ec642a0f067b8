/*
 * rover_lift_viewer.h -- C ABI of the rgb_array viewer of FrankaCubeLift-v0 (librover_hip.so): one world-placed pinhole camera
 * that renders every env's table, arm, gripper, cube and goal marker into one RGBA image.  DESIGN.md section 29 is the image
 * contract.
 *
 * Replaces the viewport camera ORBIT's RLTaskEnv.render() reads in "rgb_array" mode for this task (placed by cfg.viewer; the
 * reference sets eye = (-6, -6, 3.5), manipulation_env_cfg.py:235), which gymnasium's RecordVideo records.
 *
 * Conventions as in rover_viewer.h: plain C, caller-owned DEVICE buffers, int return codes, rover_last_error() for the text, all
 * calls asynchronous on `stream` (none allocates or synchronises).  The viewer reads the STATE BUFFER a rover_lift_sim is bound
 * to (rover_lift_bind), not the handle; the launch device is the one the state pointer lives on.
 *
 * Env placement (ASSUMED: ORBIT's grid cloner is not in the reference checkout).  The state is in the env frame (robot root at
 * the env's origin, identity orientation); env e of n is drawn at
 *     rows = ceil(n / int(sqrt(n))), cols = ceil(n / rows), row = e / cols, col = e % cols,
 *     x = (0.5 (rows - 1) - row) spacing, y = (col - 0.5 (cols - 1)) spacing, z = 0.
 */
#ifndef ROVER_LIFT_VIEWER_H
#define ROVER_LIFT_VIEWER_H

#include <stddef.h>
#include <stdint.h>

#include "rover_lift.h"
#include "rover_viewer.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rover_lift_viewer_config {
    float eye[3];                   /* m; finite.  origin_type ENV: relative to env `env_index`'s origin                      */
    float lookat[3];                /* m; finite, != eye, and lookat - eye not parallel to +Z (world +Z is up)              */
    int32_t origin_type;            /* ROVER_VIEWER_ORIGIN_WORLD (default) or ROVER_VIEWER_ORIGIN_ENV                        */
    int32_t env_index;              /* 0 <= env_index < num_envs when origin_type is ENV                                     */
    int32_t width, height;          /* pixels, 1 .. ROVER_VIEWER_MAX_SIZE (default 1280 x 720)                                */
    float focal_length;             /* mm; f = width * focal_length / horizontal_aperture pixels, square pixels              */
    float horizontal_aperture;      /* mm (defaults of rover_viewer_config: 18.147562 / 20.955, horizontal FOV 60 deg)       */
    float near_clip, far_clip;      /* m; 0 <= near_clip < far_clip, far_clip may be +inf (defaults 0.01, 1e6)               */
    int32_t draw_targets;           /* non-zero: one sphere per env at its goal (the command term's debug_vis; default 1)    */
    float env_spacing;              /* m; finite, > 0 (default 2.5, manipulation_env_cfg.py:198)                             */
    float ee_offset_z;              /* m; finite (default 0.1034, joint_pos_env_cfg.py:78): flange -> tool centre point      */
} rover_lift_viewer_config;

/* eye (-6, -6, 3.5) (manipulation_env_cfg.py:235), lookat (0, 0, 0), 1280 x 720, origin "world", Kit's default lens. */
int rover_lift_viewer_default_config(rover_lift_viewer_config *cfg);
/* sizeof(rover_lift_viewer_config): lets a binding check its mirror of the struct. */
size_t rover_lift_viewer_config_bytes(void);

/* Bytes of the caller-owned device workspace (256-byte aligned) for `num_envs` envs: the per-frame world-frame primitives and
 * bounds of every env and the overflow list.  0 if `cfg` is invalid or num_envs <= 0.  After a render the workspace's first
 * int32 holds the number of envs on the overflow list (a diagnostic: envs whose bounds leave the 3 x 3 lattice cells around
 * their own, which every ray tests; normally 0 at the default spacing). */
size_t rover_lift_viewer_workspace_bytes(int32_t num_envs, const rover_lift_viewer_config *cfg);

/* The viewer's copies of the model data it draws from (csrc/lift_render.hpp), for a check against rover_lift_model_constants:
 * [3 i + 0 .. 2] = (kind, a, d) of modified-DH row i = 0 .. 6, then K_FLANGE_D, K_CUBE_HALF, K_PAD_HALF_X, K_PAD_HALF_Z
 * (25 values).  Returns the count; writes min(count, cap) values.  Host only. */
int rover_lift_viewer_constants(float *out, int32_t cap);

/* The (num_envs, 3) env origins the render uses (formula above), into HOST memory.  Host only. */
int rover_lift_viewer_env_origins(int32_t num_envs, float env_spacing, float *out_host);

/* One frame of `state` (LIFT_STATE_WORDS x num_envs fp32 SoA, the buffer of rover_lift_bind): rgba (height, width) packed uint8
 * RGBA (alpha 255), row 0 at the top; depth (height, width) fp32 Euclidean distance to the hit (+inf: sky); object_id (height,
 * width) int32 (sky 0, ground 1, env e: 2 + 16 e + {0 table, 1..8 arm segments, 9 hand, 10 finger 0, 11 finger 1, 12 cube,
 * 13 goal}).  depth / object_id may be NULL (not written).  One pose pass and one render launch, asynchronous on `stream`;
 * the state is only read.
 * ROVER_ERR_INVALID: NULL state / ws / rgba, ws_bytes < rover_lift_viewer_workspace_bytes, ws not 256-byte aligned, a bad
 * config (including env_index out of range with origin ENV), num_envs <= 0, or a state pointer that is not device memory. */
int rover_lift_viewer_render(const float *state, int32_t num_envs, const rover_lift_viewer_config *cfg, void *ws, size_t ws_bytes,
                             uint32_t *rgba, float *depth, int32_t *object_id, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ROVER_LIFT_VIEWER_H */
