/*
 * rover_elevation_traverse.h -- C ABI of the elevation map's traversability layers: local slope, step height, roughness and a cost
 * combined from them, with the scan of the cost (librover_hip.so).
 *
 * The rolling map of rover_elevation.h and the min-fill of rover_elevation_fill.h end in a height image.  rover_elevation_traverse
 * derives from such an image where a robot may drive, the way elevation-mapping stacks do: per cell the slope of the surface, the
 * largest height difference and the roughness within a (2r + 1)^2 neighbourhood, a cost in [0, 1] and a verdict (free / lethal).
 * ONE launch per call on a read-only height image: `heights` is n x G x G floats in the map's slot order, NaN = unknown -- `map`
 * itself, or the `filled_out` of rover_elevation_fill; the launch does not care which.  It has no state.
 *
 * rover_elevation_traverse, per env e, every operation one correctly rounded fp32 operation in the order written (no contraction):
 *   1 window    as step 1 of rover_elevation_fill.h: lo = origin - G/2 (per axis); window cell (i, j), i over y and j over x, both
 *               in [0, G), is the global cell (lo.x + j, lo.y + i), stored at slot ((lo.x + j) & (G - 1), (lo.y + i) & (G - 1)) of
 *               `heights`; h[i][j] is that slot's float.  A cell is USABLE iff its float is finite: NaN and +-inf are not.
 *   2 per usable cell c = (i, j): its neighbourhood is the usable cells (i + di, j + dj) with |di|, |dj| <= r inside [0, G)^2.  The
 *               toroidal seam is no neighbourhood: window columns G - 1 and 0 are adjacent slots, not adjacent cells.
 *       support   the number of neighbourhood cells, the centre included.
 *       step      value(max key) - value(min key) over the neighbourhood, on the keys below: independent of the order, -0 < +0.
 *       gradient  on the x axis, with lower = (i, j - 1), upper = (i, j + 1), each counted only if usable (and inside the window):
 *                     both:        gx = (h[i][j+1] - h[i][j-1]) * (0.5f * inv_cell)
 *                     upper only:  gx = (h[i][j+1] - h[i][j]) * inv_cell
 *                     lower only:  gx = (h[i][j] - h[i][j-1]) * inv_cell
 *                     neither:     gx = 0
 *                 gy alike over i.  slope = sqrtf((gx * gx) + (gy * gy)): a tangent.
 *       rough     over the neighbourhood without the centre, di outer ascending, dj inner ascending, acc = 0 at first:
 *                     res = (h[i+di][j+dj] - h[i][j]) - ((gx * ((float)dj * cell)) + (gy * ((float)di * cell)));  acc = acc + res * res
 *                 cnt = support - 1;  rough = cnt == 0 ? 0 : sqrtf(acc / (float)cnt): the RMS residual of the tangent plane.
 *       lethal    !(slope < slope_crit && step < step_crit && rough < rough_crit): a NaN or an overflow from huge heights is lethal.
 *       cost      lethal ? 1.0f : fminf(((w_slope * (slope / slope_crit)) + (w_step * (step / step_crit)))
 *                                       + (w_rough * (rough / rough_crit)), 1.0f)
 *       class     lethal ? 2 : 1.
 *   3 no verdict  a cell that is not usable, or whose support < min_support: the quiet NaN 0x7FC00000 in all four layers, class 0.
 *   4 window outputs (each optional) slope_out, step_out, rough_out, cost_out: the layers in the SLOT order of `heights`.
 *   5 scan      (skipped when cost_scan_out is NULL; class_out and lethal_count_out are then not written) step 8 of
 *               rover_elevation.h on the cost window: the same yaw frame, cell() and window test, run by the same device function.
 *               A column over a cell of class 1 or 2 reads that cell's cost itself (no (pos.z - h) - height_offset); any other
 *               column reads unknown_cost.  class_out: one byte per column, 0, 1 or 2; a column outside the window or under a
 *               bad pose gets 0.  lethal_count_out: the class-2 columns of the env (an integer reduction).  A non-finite pose
 *               float gives an all-unknown row, class 0, count 0; the window outputs do not depend on the pose.
 *
 * Keys: a float's bits b become key = (b & 0x80000000) ? ~b : (b | 0x80000000), which orders as the float does (rover_elevation.h).
 *
 * The default thresholds and weights of the Python cfg class are the implementer's choice, not tuned values; nothing here says how
 * well anything drives from the cost.
 *
 * Conventions as in rover_elevation_fill.h: plain C, caller-owned DEVICE buffers, int return codes, rover_last_error() for the text,
 * asynchronous on `stream`, run on the device `heights` lives on; one launch, no workspace, no allocation, no host synchronisation;
 * the arguments are checked before the device is looked at.
 */
#ifndef ROVER_ELEVATION_TRAVERSE_H
#define ROVER_ELEVATION_TRAVERSE_H

#include <stddef.h>
#include <stdint.h>

#include "rover_elevation.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ROVER_ELEVATION_TRAVERSE_MAX_RADIUS 4

typedef struct rover_elevation_traverse_cfg {
    int32_t radius;                            /* r in [1, 4]: the neighbourhood is (2r + 1)^2 cells                        */
    int32_t min_support;                       /* in [1, (2r + 1)^2]: usable cells (centre included) a cell needs           */
    float slope_crit, step_crit, rough_crit;   /* finite, > 0; slope is a tangent, the others metres                        */
    float w_slope, w_step, w_rough;            /* finite, >= 0, the fp32 sum ((w_slope + w_step) + w_rough) <= 1            */
    float unknown_cost;                        /* not a NaN: what a scan column without a cost reads                        */
} rover_elevation_traverse_cfg;

size_t rover_elevation_traverse_cfg_bytes(void);

/* One launch: steps 1 - 5 above for envs e < n.
 *   cfg, t         HOST structs, copied before the call returns; cfg as rover_elevation_scan takes it.
 *   pos, quat, comp_stride, env_stride, origin, ray_x, nx, ray_y, ny, scan_pitch
 *                  as in rover_elevation_fill; cost_scan_out (n rows of nx * ny floats, scan_pitch floats apart) may be NULL: then
 *                  there is no scan, class_out and lethal_count_out are not written, and ray_x and ray_y may be NULL.
 *   heights        n * grid * grid floats, read only; origin read only.
 *   class_out      NULL or n * nx * ny bytes; lethal_count_out NULL or n int32.
 *   slope_out, step_out, rough_out, cost_out   each NULL or n * grid * grid floats.  One of cost_scan_out and these four is required.
 * ROVER_ERR_UNSUPPORTED, and nothing launched, for: grid not a power of two in [8, 128]; nx * ny > 4096.
 * ROVER_ERR_INVALID, and nothing launched, for: a NULL cfg, t, pos, quat, heights or origin; cost_scan_out and the four window
 * outputs all NULL; cost_scan_out without ray_x or ray_y; radius outside [1, 4]; min_support outside [1, (2r + 1)^2]; a crit that is
 * not finite and > 0; a weight that is not finite and >= 0, or their fp32 sum above 1; a NaN unknown_cost; n, comp_stride,
 * env_stride, nx or ny <= 0; a float or int32 pointer that is not 4-byte aligned; scan_pitch < nx * ny; the cfg values
 * rover_elevation_scan refuses; an output overlapping heights. */
int rover_elevation_traverse(const rover_elevation_cfg *cfg, const rover_elevation_traverse_cfg *t, const float *pos,
                             const float *quat, int64_t comp_stride, int64_t env_stride, const float *heights, const int32_t *origin,
                             const float *ray_x, int32_t nx, const float *ray_y, int32_t ny, float *cost_scan_out, int64_t scan_pitch,
                             uint8_t *class_out, int32_t *lethal_count_out, float *slope_out, float *step_out, float *rough_out,
                             float *cost_out, int32_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_ELEVATION_TRAVERSE_H */
