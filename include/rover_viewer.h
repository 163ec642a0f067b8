/*
 * rover_viewer.h -- C ABI of the rgb_array viewer (librover_hip.so): one world-placed pinhole camera that renders the terrain,
 * every env's rover and (optionally) every env's target into one RGBA image.  DESIGN.md section 11 is the image contract.
 *
 * Replaces the viewport camera ORBIT's RLTaskEnv.render() reads in "rgb_array" mode (placed by cfg.viewer: eye, lookat,
 * resolution; the reference sets eye = (-6, -6, 3.5), rover_env_cfg.py:272), which gymnasium's RecordVideo records.
 *
 * Conventions as in rover_camera.h: plain C, caller-owned DEVICE buffers, int return codes, rover_last_error() for the text, all
 * calls asynchronous on `stream` (none allocates or synchronises).  The viewer reads the state and terrain of a rover_sim
 * handle; it has no handle of its own.
 */
#ifndef ROVER_VIEWER_H
#define ROVER_VIEWER_H

#include <stddef.h>
#include <stdint.h>

#include "rover_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ROVER_VIEWER_ORIGIN_WORLD = 0, ROVER_VIEWER_ORIGIN_ENV = 1 };
#define ROVER_VIEWER_MAX_SIZE 8192

typedef struct rover_viewer_config {
    float eye[3];                   /* m; finite.  origin_type ENV: relative to env `env_index`'s root position (ROVER_POS) */
    float lookat[3];                /* m; finite, != eye, and lookat - eye not parallel to +Z (world +Z is up)              */
    int32_t origin_type;            /* ROVER_VIEWER_ORIGIN_WORLD (default) or ROVER_VIEWER_ORIGIN_ENV                        */
    int32_t env_index;              /* 0 <= env_index < num_envs when origin_type is ENV                                     */
    int32_t width, height;          /* pixels, 1 .. ROVER_VIEWER_MAX_SIZE (default 1280 x 720, ORBIT's ViewerCfg)             */
    float focal_length;             /* mm; f = width * focal_length / horizontal_aperture pixels, square pixels              */
    float horizontal_aperture;      /* mm (defaults: Kit's /OmniverseKit_Persp, 18.147562 / 20.955: horizontal FOV 60 deg)   */
    float near_clip, far_clip;      /* m; 0 <= near_clip < far_clip, far_clip may be +inf (defaults 0.01, 1e6)               */
    int32_t draw_targets;           /* non-zero: one sphere per env at its target (ORBIT's debug_vis; default 1)             */
} rover_viewer_config;

/* ORBIT's ViewerCfg defaults (eye (7.5, 7.5, 7.5), lookat (0, 0, 0), 1280 x 720, origin "world") and Kit's default lens. */
int rover_viewer_default_config(rover_viewer_config *cfg);
/* sizeof(rover_viewer_config): lets a binding check its mirror of the struct. */
size_t rover_viewer_config_bytes(void);

/* Bytes of the caller-owned device workspace (256-byte aligned) for `sim`'s terrain and env count: the terrain's max-height
 * pyramid and the per-frame bins of rovers and targets.  0 if no terrain is bound or `cfg` is invalid. */
size_t rover_viewer_workspace_bytes(const struct rover_sim *sim, const rover_viewer_config *cfg);

/* Build the pyramid of the terrain bound to `sim` into `ws`.  Once per bound terrain: again after every rover_set_terrain*. */
int rover_viewer_prepare(struct rover_sim *sim, const rover_viewer_config *cfg, void *ws, size_t bytes, void *stream);

/* One frame of the state `sim` holds: rgba (height, width) packed uint8 RGBA (alpha 255), row 0 at the top; depth (height,
 * width) fp32 Euclidean distance to the hit (+inf: sky); object_id (height, width) int32 (sky 0, ground 1, rock 2, env e:
 * 3 + 8 e + {0 chassis, 1..6 wheels FL FR CL CR RL RR, 7 target}).  depth / object_id may be NULL (not written).
 * A per-frame binning pass and one render launch, asynchronous on `stream`.
 * ROVER_ERR_INVALID: bad config (including env_index out of range with origin ENV) or NULL rgba / ws.
 * ROVER_ERR_STATE: no terrain or state bound, terrain re-bound since rover_viewer_prepare (or `ws` is not the prepared
 * workspace), or called between rover_step_begin and rover_step_finish. */
int rover_viewer_render(struct rover_sim *sim, const rover_viewer_config *cfg, void *ws, uint32_t *rgba, float *depth,
                        int32_t *object_id, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ROVER_VIEWER_H */
