/*
 * rover_elevation.h -- C ABI of the rolling, robot-centric elevation map built from the on-board depth camera (librover_hip.so).
 *
 * The policy reads a height scan around the rover.  The simulator's scan is an oracle (vertical rays with perfect knowledge all
 * round); a real rover builds a robot-centric elevation map from depth and odometry and reads the scan out of that map.
 * rover_elevation_step is that link as ONE launch per env step: scroll the map to the new pose, unproject the depth image, reduce
 * it to one height per cell, fuse it into the map, and read the policy's scan out of the result.
 *
 * State per env: `map`, grid x grid fp32 indexed [slot_y][slot_x], world heights in metres, NaN = unknown; `origin`, two int32,
 * the centre cell (x, y) of the last update.  Cells are anchored to the WORLD:
 *     cell(v) = (int32) fminf(fmaxf(floorf(v * inv_cell), -2^30), 2^30)          (floorf, not truncation; v finite)
 * world point (x, y) lies in global cell (gx, gy) = (cell(x), cell(y)), which is stored at slot (gx & (grid - 1), gy & (grid - 1)):
 * the addressing is toroidal, the map scrolls without moving data.  The window of centre cell c covers [c - grid/2, c + grid/2)
 * on each axis; slot s of a window with low corner lo denotes the global cell lo + ((s - lo) & (grid - 1)).
 *
 * rover_elevation_step, per env, every product and sum one fp32 operation rounded once (no contraction), in this order:
 *   1 reset     flag = (reset_a && reset_a[e]) || (reset_b && reset_b[e]): the old map counts as all unknown.
 *   2 bad pose  if one of the seven pose floats is not finite: `map` and `origin` stay as they are (with the flag set, `map` is
 *               written all NaN), the scan row is all unknown_value, known 0, count 0; nothing else happens for this env.
 *   3 scroll    c = (cell(pos.x), cell(pos.y)).  A slot keeps its old value only if the global cell it denotes in the window of c
 *               is the one it denoted in the window of `origin`; otherwise it becomes unknown.
 *   4 unproject (skipped when depth is NULL) pixel k with depth d is valid if d is finite and range_min <= d <= range_max.  With
 *               (rx, ry, rz) = ray_b[k], m = mount_pos and (w, x, y, z) = quat AS STORED (not renormalised):
 *                   bx = m[0] + d * rx;  by = m[1] + d * ry;  bz = m[2] + d * rz
 *                   r00 = 1 - 2 * (y*y + z*z);  r01 = 2 * (x*y - w*z);  r02 = 2 * (x*z + w*y)
 *                   r10 = 2 * (x*y + w*z);  r11 = 1 - 2 * (x*x + z*z);  r12 = 2 * (y*z - w*x)
 *                   r20 = 2 * (x*z - w*y);  r21 = 2 * (y*z + w*x);  r22 = 1 - 2 * (x*x + y*y)
 *                   px = pos.x + ((r00 * bx + r01 * by) + r02 * bz)        (py, pz alike with rows 1 and 2)
 *               A point with a non-finite coordinate, or whose cell lies outside the window, is dropped.
 *   5 reduce    frame value of a cell = the maximum pz over this frame's points in the cell, in the order of the keys below
 *               (-0 < +0); a maximum does not depend on the order of the points, so the result is bit-reproducible.
 *   6 fuse      untouched cell: its scrolled value.  Touched and unknown (NaN): the frame value.  Touched and known:
 *               alpha == 1 ? frame : old + alpha * (frame - old).  A NaN result is written as the quiet NaN 0x7FC00000.
 *   7 store     `map` and `origin` (= c) are written back.
 *   8 scan      (skipped when scan_out is NULL; known_out and count_out are then not written either) for ray (i, j), i over
 *               ray_y, j over ray_x, column i * nx + j, with ox = ray_x[j], oy = ray_y[i]:
 *                   a = 1 - 2 * (y*y + z*z);  b = 2 * (w*z + x*y);  inv = 1 / sqrtf(a*a + b*b);  cy = a * inv;  sy = b * inv
 *                   sx_ = pos.x + (cy * ox - sy * oy);  sy_ = pos.y + (sy * ox + cy * oy)
 *               (the yaw frame of the height scanner, division and square root correctly rounded).  If both are finite and their
 *               cell lies in the map's window and is known with height h, the column is (pos.z - h) - height_offset and counts as
 *               known; otherwise it is unknown_value.  known_out: one byte per column (0 / 1); count_out: the known columns of the
 *               env (an integer reduction).
 * rover_elevation_scan is step 8 alone on a read-only map, for any poses: the window is that of the stored `origin`; a non-finite
 * pose gives an all-unknown row.  Both entry points run the same device function, so they agree on the bits.
 *
 * Keys (step 5): a float's bits b become key = (b & 0x80000000) ? ~b : (b | 0x80000000), which orders as the float does; 0 is
 * never the key of a finite float and stands for "untouched".  The reduction is an LDS unsigned-max atomic: no float atomics.
 *
 * Conventions as in rover_depth_sensor.h: plain C, caller-owned DEVICE buffers, int return codes, rover_last_error() for the text,
 * asynchronous on `stream` and run on the device `map` lives on.  One launch; no workspace, no allocation, no host synchronisation.
 * The arguments are checked before the device is looked at, so every refusal below also works on a host without a GPU.
 */
#ifndef ROVER_ELEVATION_H
#define ROVER_ELEVATION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ROVER_ELEVATION_MIN_GRID 8
#define ROVER_ELEVATION_MAX_GRID 128          /* one map is at most 64 KB of LDS */
#define ROVER_ELEVATION_MAX_PIXELS 16384
#define ROVER_ELEVATION_MAX_RAYS 4096

typedef struct rover_elevation_cfg {
    float cell, inv_cell;                /* metres per cell and the caller's fp32 of 1 / cell; both finite and > 0   */
    int32_t grid;                        /* G: cells per side, a power of two in [8, 128]                            */
    float range_min, range_max;          /* metres; 0 < range_min <= range_max, range_max may be +inf                */
    float alpha;                         /* weight of the new frame on a known cell, in (0, 1]                       */
    float mount_pos[3];                  /* the optical centre in the Body frame, metres                             */
    float height_offset;                 /* the height scanner's offset                                              */
    float unknown_value;                 /* what an unknown scan column reads; not NaN                               */
} rover_elevation_cfg;

size_t rover_elevation_cfg_bytes(void);

/* One launch: steps 1 - 8 above for envs e < n.
 *   cfg            HOST struct; it is copied before the call returns.
 *   depth          NULL (no frame: scroll and scan only), or device floats, image e at depth + e * pitch_floats, row-major
 *                  height x width; 4-byte aligned (16-byte accesses where the offset allows, same values either way).
 *   ray_b          height * width unit directions (x, y, z) in the Body frame, mount rotation applied; required with depth.
 *   pos, quat      component c of env e at pos[e * env_stride + c * comp_stride], quat (w, x, y, z) alike under the same two
 *                  strides (in floats, both > 0): (n, 1) reads the SoA state rows as they are, (1, 7) an AoS array of
 *                  (x, y, z, w, qx, qy, qz) poses with quat = pos + 3.
 *   reset_a/b      each NULL or n bytes, OR-ed.
 *   map, origin    n * grid * grid floats and n * 2 int32, read and written in place.
 *   ray_x, ray_y   nx and ny offsets (metres, rover yaw frame) of the scan's columns and rows.
 *   scan_out       NULL, or row e at scan_out + e * scan_pitch, nx * ny floats; the pitch's gap is neither read nor written.
 *   known_out      NULL or n * nx * ny bytes; count_out NULL or n int32.
 * ROVER_ERR_UNSUPPORTED, and nothing launched, for: grid not a power of two in [8, 128]; height * width > 16384; nx * ny > 4096.
 * ROVER_ERR_INVALID, and nothing launched, for: a NULL cfg, pos, quat, map, origin, ray_x or ray_y; depth without ray_b; n <= 0;
 * height, width, nx, ny, comp_stride or env_stride <= 0; a float or int32 pointer that is not 4-byte aligned; pitch_floats <
 * height * width; scan_pitch < nx * ny; cell or inv_cell not finite and positive; range_min not > 0, not finite or above range_max
 * (a NaN range_max included); alpha outside (0, 1]; a NaN unknown_value or height_offset; a non-finite mount_pos; map overlapping
 * scan_out or depth. */
int rover_elevation_step(const rover_elevation_cfg *cfg, const float *depth, int64_t pitch_floats, int32_t height, int32_t width,
                         const float *ray_b, const float *pos, const float *quat, int64_t comp_stride, int64_t env_stride,
                         const uint8_t *reset_a, const uint8_t *reset_b, float *map, int32_t *origin, const float *ray_x,
                         int32_t nx, const float *ray_y, int32_t ny, float *scan_out, int64_t scan_pitch, uint8_t *known_out,
                         int32_t *count_out, int32_t n, void *stream);

/* Step 8 alone; `map` and `origin` are only read, scan_out is required.  Refusals as above (no depth, ray_b or reset here). */
int rover_elevation_scan(const rover_elevation_cfg *cfg, const float *pos, const float *quat, int64_t comp_stride,
                         int64_t env_stride, const float *map, const int32_t *origin, const float *ray_x, int32_t nx,
                         const float *ray_y, int32_t ny, float *scan_out, int64_t scan_pitch, uint8_t *known_out,
                         int32_t *count_out, int32_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ROVER_ELEVATION_H */
