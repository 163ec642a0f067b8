/*
 * rover_lidar.h -- C ABI of the rover's scanning lidar (librover_hip.so): a cast of an arbitrary table of Body-frame rays from
 * each env's pose against the terrain's triangle mesh.
 *
 * The reference's only range sensor beside the camera is the height scanner, an ORBIT RayCaster with the grid pattern
 * (rover_envs/envs/navigation/rover_env_cfg.py:78-86).  ORBIT's RayCaster offers lidar patterns next to it (patterns.LidarPatternCfg);
 * this is that sensor: `range` is the length of ORBIT's ray to its hit, `hits_w` its `ray_hits_w`.  The geometry is the mesh of
 * rover_camera.h (the heightfield bound by rover_set_terrain, cells split along the (i, j) - (i+1, j+1) diagonal) and the march is
 * the camera's (csrc/terrain_march.hpp); what differs is where the rays come from -- a caller-supplied table, not a lens -- and
 * which rays share a wave: 64 CONSECUTIVE table entries of one env.  The order of the table is the caller's, so the caller decides
 * which rays march together.
 *
 * rover_lidar_cast, per env e and table entry k < rays, every product and sum one fp32 operation rounded once (no contraction),
 * division and square root correctly rounded, in this order, with pos and (w, x, y, z) = quat the env's state words:
 *   1 normalise   s = ((w*w + x*x) + y*y) + z*z;  inv = 1 / sqrtf(s);  w = w * inv;  x = x * inv;  y = y * inv;  z = z * inv
 *                 (the camera kernel's normalisation)
 *   2 frame       attach_yaw_only == 0, the full attitude:
 *                     r00 = 1 - 2 * (y*y + z*z);  r01 = 2 * (x*y - w*z);  r02 = 2 * (x*z + w*y)
 *                     r10 = 2 * (x*y + w*z);  r11 = 1 - 2 * (x*x + z*z);  r12 = 2 * (y*z - w*x)
 *                     r20 = 2 * (x*z - w*y);  r21 = 2 * (y*z + w*x);  r22 = 1 - 2 * (x*x + y*y)
 *                 attach_yaw_only == 1, the yaw frame, (cy, sy) formed as rover_elevation.h step 8 forms them, here from the
 *                 normalised quaternion:
 *                     a = 1 - 2 * (y*y + z*z);  b = 2 * (w*z + x*y);  i2 = 1 / sqrtf(a*a + b*b);  cy = a * i2;  sy = b * i2
 *                     r00 = cy;  r01 = -sy;  r02 = 0;   r10 = sy;  r11 = cy;  r12 = 0;   r20 = 0;  r21 = 0;  r22 = 1
 *   3 origin      with m = mount_pos:  o_i = pos_i + ((r_i0 * m[0] + r_i1 * m[1]) + r_i2 * m[2])             (i = 0, 1, 2)
 *   4 direction   with (rx, ry, rz) = ray_b[k]:  d_i = (r_i0 * rx + r_i1 * ry) + r_i2 * rz
 *   5 march       range[e * pitch_floats + k] = the first t in [near_clip, far_clip] at which o + t d meets the mesh, +inf where
 *                 there is none (the ray leaves the terrain, climbs above its highest point or passes far_clip).  A non-finite
 *                 pose or ray gives a miss: the marcher refuses a non-finite origin or direction.  The march needs a finite end
 *                 of its range: a ray with d_x = d_y = 0 EXACTLY and d_z < 0 finds it only in far_clip, so under
 *                 far_clip = +inf the result of such a ray is not specified (as a rule a miss; a limit of the shared marcher,
 *                 the camera's too).  Give a finite far_clip where the table holds the Body's -z and the rover may stand level.
 *   6 hit         (hits_w != NULL)  hits_w[(e * rays + k) * 3 + i] = o_i + range * d_i, the product rounded, then the sum; on a
 *                 miss all three components are +inf.
 * The gap of the pitch, range[e * pitch_floats + rays ...], is neither read nor written.  All offsets are 64-bit.
 *
 * Workspace: the max-height pyramid of rover_camera.h, the same bytes in the same layout.  rover_lidar_prepare and
 * rover_camera_prepare write the same record in the handle, so ONE prepared workspace serves rover_camera_render and
 * rover_lidar_cast alike, whichever call prepared it, and the last prepare wins: a workspace prepared earlier at another address
 * is refused by both until it is prepared again.
 *
 * Conventions as in rover_camera.h and rover_elevation.h: plain C, caller-owned DEVICE buffers, int return codes,
 * rover_last_error() for the text, asynchronous on `stream`; the calls read the state and terrain of a rover_sim handle and run on
 * the handle's device.  Every ROVER_ERR_INVALID below is decided from the arguments alone, before the handle or the device is
 * looked at, so those refusals also work on a host without a GPU.
 */
#ifndef ROVER_LIDAR_H
#define ROVER_LIDAR_H

#include <stddef.h>
#include <stdint.h>

#include "rover_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* word 3 of the Philox counter of the noise on a lidar frame (rover_obs_post.h's `tag` argument): "OL" in the high half, beside
 * "OP" (observation rows) and "OD" (depth images) */
#define ROVER_LIDAR_STREAM_NOISE 0x4F4C0000u

typedef struct rover_lidar_config {
    int32_t rays;                 /* R >= 1: entries of the table                                                       */
    float   mount_pos[3];         /* m, the sensor's origin in the Body frame; finite                                   */
    float   near_clip, far_clip;  /* m; 0 <= near_clip < far_clip, far_clip may be +inf (ORBIT's max_distance)          */
    int32_t attach_yaw_only;      /* 0: the table turns with the full attitude; 1: with the yaw frame only (step 2)     */
} rover_lidar_config;

/* sizeof(rover_lidar_config): lets a binding check its mirror of the struct. */
size_t rover_lidar_config_bytes(void);

/* Bytes of the workspace for the terrain bound to `sim` (= rover_camera_workspace_bytes of any valid camera config); 0 if `sim`
 * is NULL or no terrain is bound. */
size_t rover_lidar_workspace_bytes(const struct rover_sim *sim);

/* Build the pyramid of the terrain currently bound to `sim` into `ws` (256-byte aligned, `bytes` >= rover_lidar_workspace_bytes).
 * Call again after every rover_set_terrain* on `sim`.  ROVER_ERR_INVALID: NULL sim / ws, ws misaligned or too small;
 * ROVER_ERR_STATE: no terrain bound. */
int rover_lidar_prepare(struct rover_sim *sim, void *ws, size_t bytes, void *stream);

/* One launch: steps 1 - 6 above for every env of `sim`.
 *   ray_b         cfg->rays * 3 floats, unit directions (x, y, z) in the Body frame -- the table rover_elevation_step consumes,
 *                 so one device buffer serves both calls.
 *   range         row e at range + e * pitch_floats, cfg->rays floats.
 *   hits_w        NULL (nothing is written), or num_envs * cfg->rays * 3 floats.
 * ROVER_ERR_INVALID, and nothing launched, for: a NULL sim, cfg, ws, ray_b or range; rays <= 0; pitch_floats < rays or > 2^29 (any
 * number of rows then stays inside 64-bit byte offsets); ray_b, range or hits_w not 4-byte aligned; a non-finite mount_pos; near_clip
 * negative, not below far_clip, or either of them a NaN; attach_yaw_only not 0 or 1.
 * ROVER_ERR_STATE, as rover_camera_render: no terrain or state bound; `ws` not the workspace prepared for the terrain bound now;
 * called between rover_step_begin and rover_step_finish.
 * ROVER_ERR_UNSUPPORTED: num_envs * ceil(rays / 64) waves are more than one launch's grid holds. */
int rover_lidar_cast(struct rover_sim *sim, const rover_lidar_config *cfg, const void *ws, const float *ray_b, float *range,
                     int64_t pitch_floats, float *hits_w, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ROVER_LIDAR_H */
