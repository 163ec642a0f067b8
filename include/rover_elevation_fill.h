/*
 * rover_elevation_fill.h -- C ABI of the elevation map's inpainting pass: a conservative minimum fill with a fill-distance scan
 * (librover_hip.so).
 *
 * The rolling map of rover_elevation.h knows only the cells its sensor has swept; a scan column over any other cell reads
 * unknown_value, which the policy takes for ground at exactly height_offset below the body.  rover_elevation_fill closes the holes
 * the way elevation-mapping stacks do: unknown cells take a value from their known neighbours, ring by ring, and every value
 * carries how far it was carried.  The value is the MINIMUM of the neighbours (occluded ground is usually lower than what occludes
 * it).  ONE launch per call, on a copy of the map's window; `map` and `origin` are read and never written, the fill has no state.
 *
 * rover_elevation_fill, per env e, in this order:
 *   1 window    lo = origin - G/2 (per axis).  Window cell (i, j), i over y and j over x, both in [0, G), is the global cell
 *               (lo.x + j, lo.y + i), stored at slot ((lo.x + j) & (G - 1), (lo.y + i) & (G - 1)) of `map` ([slot_y][slot_x]).
 *               h0[i][j] is that slot's float; dist0[i][j] = isnan(h0[i][j]) ? 255 : 0.  Only a NaN is unknown (+-inf is a height).
 *   2 fill      for k = 1 ... iterations: every cell with dist == 255 looks at its 8 window neighbours (i + di, j + dj).  A
 *               neighbour counts if it lies inside [0, G)^2 and has dist < k.  The toroidal seam is no neighbourhood: window
 *               columns G - 1 and 0 are adjacent slots, not adjacent cells.  If no neighbour counts the cell stays as it is;
 *               otherwise it takes the minimum of the counting neighbours' heights in the order of the keys below (-0 < +0; the
 *               bits of one of them, no arithmetic) and dist = k.  Sweep k reads only what sweeps < k produced (a Jacobi sweep),
 *               so the result does not depend on the order of the cells and is bit-reproducible: after the sweeps, dist of a
 *               filled cell is its Chebyshev distance, within the window, to the nearest measured cell.  The kernel stops once
 *               a sweep fills nothing; the result is the same.
 *   3 window outputs (each optional) filled_out: the filled heights in the map's own SLOT order, a cell that is still unknown
 *               and a measured cell bit-equal to `map`; dist_out: the dist bytes in the same order.
 *   4 scan      (skipped when scan_out is NULL; scan_dist_out and count_out are then not written) step 8 of rover_elevation.h on
 *               the filled window: the same yaw frame, cell(), window test and (pos.z - h) - height_offset.  A column over a cell
 *               with dist < 255 reads that cell's height, any other column unknown_value.  scan_dist_out: one byte per column,
 *               0 = measured, k = filled in sweep k, 255 = unknown, outside the window or a bad pose.  count_out: the columns
 *               with dist < 255.  A non-finite pose float gives an all-unknown row, dist 255, count 0; the window outputs of
 *               step 3 do not depend on the pose and are written all the same.  A column with dist 0 is bit-equal to what
 *               rover_elevation_scan gives for the same map and pose: both run the same device function.
 *
 * Keys: a float's bits b become key = (b & 0x80000000) ? ~b : (b | 0x80000000), which orders as the float does (rover_elevation.h).
 *
 * Conventions as in rover_elevation.h: plain C, caller-owned DEVICE buffers, int return codes, rover_last_error() for the text,
 * asynchronous on `stream`, run on the device `map` lives on; one launch, no workspace, no allocation, no host synchronisation;
 * the arguments are checked before the device is looked at.
 */
#ifndef ROVER_ELEVATION_FILL_H
#define ROVER_ELEVATION_FILL_H

#include <stddef.h>
#include <stdint.h>

#include "rover_elevation.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ROVER_ELEVATION_FILL_MAX_ITERATIONS 254      /* dist is one byte, 255 stands for unknown */

typedef struct rover_elevation_fill_cfg {
    int32_t iterations;                  /* sweeps, in [1, 254]: how many cells a height is carried at the most */
} rover_elevation_fill_cfg;

size_t rover_elevation_fill_cfg_bytes(void);

/* One launch: steps 1 - 4 above for envs e < n.
 *   cfg, fill      HOST structs, copied before the call returns; cfg as rover_elevation_scan takes it.
 *   pos, quat, comp_stride, env_stride, map, origin, ray_x, nx, ray_y, ny, scan_out, scan_pitch, count_out
 *                  as in rover_elevation_scan, but scan_out may be NULL: then there is no scan, scan_dist_out and count_out are
 *                  not written, and ray_x and ray_y may be NULL.
 *   scan_dist_out  NULL or n * nx * ny bytes.
 *   filled_out     NULL or n * grid * grid floats; dist_out NULL or n * grid * grid bytes.  One of scan_out and filled_out is
 *                  required.
 * ROVER_ERR_UNSUPPORTED, and nothing launched, for: grid not a power of two in [8, 128]; nx * ny > 4096.
 * ROVER_ERR_INVALID, and nothing launched, for: a NULL cfg, fill, pos, quat, map or origin; scan_out and filled_out both NULL;
 * scan_out without ray_x or ray_y; iterations outside [1, 254]; n, comp_stride, env_stride, nx or ny <= 0; a float or int32 pointer
 * that is not 4-byte aligned; scan_pitch < nx * ny; the cfg values rover_elevation_scan refuses; filled_out overlapping map or
 * scan_out. */
int rover_elevation_fill(const rover_elevation_cfg *cfg, const rover_elevation_fill_cfg *fill, const float *pos, const float *quat,
                         int64_t comp_stride, int64_t env_stride, const float *map, const int32_t *origin, const float *ray_x,
                         int32_t nx, const float *ray_y, int32_t ny, float *scan_out, int64_t scan_pitch, uint8_t *scan_dist_out,
                         int32_t *count_out, float *filled_out, uint8_t *dist_out, int32_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_ELEVATION_FILL_H */
