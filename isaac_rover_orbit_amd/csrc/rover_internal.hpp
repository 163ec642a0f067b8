// rover_internal.hpp -- symbols shared between the translation units of librover_hip.so (not part of the C ABI).
#pragma once

// records the text rover_last_error() returns on this thread and hands `code` back
__attribute__((visibility("hidden"))) int rover_internal_fail(int code, const char *fmt, const char *detail = "");

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "../../include/rover_hip.h"

// The HIP device `p` lives on, for the DeviceGuard of an entry point.  A failed query also stays on the runtime's record as the
// thread's last error; with `clear_error` it is taken off, so that a later launched() does not report it (the scaler and the
// tracker ask for that).
inline int device_of(const void *p, int *dev, bool clear_error = false)
{
    hipPointerAttribute_t at;
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        if (clear_error) (void)hipGetLastError();
        return rover_internal_fail(ROVER_ERR_INVALID, "not a device pointer: %s", hipGetErrorString(e));
    }
    *dev = at.device;
    return ROVER_OK;
}
// after a launch: the runtime's last error under the entry point's format string `what`, or ROVER_OK
inline int launched(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, what, hipGetErrorString(e));
    return ROVER_OK;
}

// in an entry point: a failed HIP call is the entry's ROVER_ERR_HIP, with the call's text and the runtime's message
#define HIP_TRY(expr)                                                                                                  \
    do {                                                                                                               \
        hipError_t _e = (expr);                                                                                        \
        if (_e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, #expr ": %s", hipGetErrorString(_e));         \
    } while (0)

// Every entry point that launches work runs on the handle's device, whatever the calling thread's current device is.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (switched) (void)hipSetDevice(prev);
    }
};

struct rover_sim;
// What another translation unit (camera_kernels.hip) may read of a handle: its device, its bound state and terrain, the
// call-order flags and the terrain generation (bumped by every rover_set_terrain*), plus the bookkeeping the handle keeps for
// the camera and the viewer: which workspace was prepared for which terrain generation.
struct rover_sim_view {
    int device;              // the handle's HIP device (DeviceGuard)
    const float *state;      // SoA state words, state[word * n + env]; NULL before rover_bind
    int n;
    bool have_terrain, phase_open;
    const float *height;     // (H, W) fp32 heightfield, row = y
    const float *obstacle;   // (H, W) fp32 obstacle layer (rock height above the ground), row = y
    int H, W;
    float res, min_x, min_y;
    uint64_t terrain_gen;
    const void **camera_ws;  // the handle's record of the last rover_camera_prepare
    uint64_t *camera_gen;
    const void **viewer_ws;  // ... and of the last rover_viewer_prepare
    uint64_t *viewer_gen;
};
__attribute__((visibility("hidden"))) rover_sim_view rover_internal_view(rover_sim *sim);
// camera_kernels.hip: the terrain's max-height pyramid (terrain_march.hpp layout) into `ws`, asynchronously on `stream`
__attribute__((visibility("hidden"))) int rover_internal_build_pyramid(const rover_sim_view &s, void *ws, void *stream);
