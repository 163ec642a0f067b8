// depth_sensor_kernels.hip -- the depth camera's sensor model (range, edge-aware dropout, axial noise, disparity steps) as one launch
// (gfx950 / CDNA4, wave64).
//
// See include/rover_depth_sensor.h for the contract, the per-pixel sequence and the draw addressing.  One kernel:
//   depth_sensor_kernel   one workgroup of 512 threads per image.  It stages the whole image into LDS (pixel p at float p: 16-byte
//                         loads and LDS stores, eight in flight per thread, when the image starts on a 16-byte boundary, dword by
//                         dword otherwise), passes one barrier, and only then writes: that is the in-place rule, every read of
//                         `src` has landed before the first store to `dst`.  Behind the barrier a thread owns Philox quads of the
//                         flat pixel index: the four pixels 4 q .. 4 q + 3 come from LDS as one 16-byte read, their up / down
//                         neighbours as one 16-byte read each where width % 4 == 0 (dword reads otherwise: a quad then crosses row
//                         ends), left / right as one dword each.  Two Philox calls per quad (normals; uniforms only when a dropout
//                         probability is > 0, which also gates the neighbour reads), the arithmetic of the header, and one 16-byte
//                         store where `dst + 4 q` is 16-byte aligned.
//                         valid_out: a ballot / popcount per pixel slot into a wave-uniform counter, one LDS int per wave, summed
//                         by thread 0.  No atomics.
// LDS: 16388 floats of image (the limit plus the pad the last quad's right neighbour reads) + 8 wave counters = 65584 bytes: two
// workgroups per CU, four waves per SIMD.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/rover_hip.h"
#include "../../include/rover_depth_sensor.h"
#include "rover_internal.hpp"
#include "train_math.hpp"   // philox4x32, unit_uniform, box_muller

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int TT = 512;
constexpr int WAVES = TT / 64;
constexpr int MAX_PIXELS = ROVER_DEPTH_SENSOR_MAX_PIXELS;
constexpr int STAGE = MAX_PIXELS / 4 / TT;      // 16-byte loads a thread keeps in flight: 8
constexpr int LDS_FLOATS = MAX_PIXELS + 4;      // the last quad's right neighbour reads float 4 q + 4

struct SensorArgs {
    rover_depth_sensor_cfg cfg;
    const float *src;
    float *dst;
    int32_t *valid_out;
    long long pitch;              // floats between two images
    unsigned long long id0;       // env_id_offset
    int height, width, hw;
    uint32_t k0, k1, c1, c2;
};

__device__ __forceinline__ bool in_range(float z, const rover_depth_sensor_cfg &c) { return z >= c.range_min && z <= c.range_max; }

// step 2 for one neighbour of a valid pixel
__device__ __forceinline__ bool edge_to(float z, float zn, const rover_depth_sensor_cfg &c)
{
    return in_range(zn, c) ? fabsf(__fsub_rn(z, zn)) > __fmul_rn(c.edge_rel, fminf(z, zn)) : c.edge_at_invalid != 0;
}

__global__ __launch_bounds__(TT) void depth_sensor_kernel(SensorArgs A)
{
    __shared__ __attribute__((aligned(16))) float img[LDS_FLOATS];
    __shared__ int wave_valid[WAVES];
    const rover_depth_sensor_cfg &cfg = A.cfg;
    const int tid = threadIdx.x, hw = A.hw, W = A.width, H = A.height;
    const size_t at = (size_t)blockIdx.x * (size_t)A.pitch;
    const float *src = A.src + at;
    float *dst = A.dst + at;

    // ---- the whole image into LDS, then one barrier: nothing below reads `src` again
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const int nv = hw >> 2;
        v4f held[STAGE];
#pragma unroll
        for (int k = 0; k < STAGE; ++k) {
            const int i = tid + k * TT;
            if (i < nv) held[k] = *reinterpret_cast<const v4f *>(src + 4 * i);
        }
#pragma unroll
        for (int k = 0; k < STAGE; ++k) {
            const int i = tid + k * TT;
            if (i < nv) *reinterpret_cast<v4f *>(img + 4 * i) = held[k];
        }
        if (tid < (hw & 3)) img[4 * nv + tid] = src[4 * nv + tid];
    } else {
        for (int p = tid; p < hw; p += TT) img[p] = src[p];
    }
    __syncthreads();

    const bool drops = cfg.p_drop > 0.0f || cfg.p_edge > 0.0f;      // u < 0 never holds: no uniforms, no neighbours
    const bool rows4 = (W & 3) == 0;                                // a quad then lies inside one row, as do its up / down quads
    const bool steps = cfg.disparity_step > 0.0f;
    const int nq = (hw + 3) >> 2;
    const uint32_t c0 = (uint32_t)(A.id0 + blockIdx.x);
    int count = 0;                                                  // wave-uniform
    for (int base = tid & ~63; base < nq; base += TT) {             // wave-uniform trip count
        const int q = base + (tid & 63);
        const int p0 = 4 * q;
        bool valid[4] = {false, false, false, false};
        if (q < nq) {
            const v4f cq = *reinterpret_cast<const v4f *>(img + p0);
            const float z0[4] = {cq.x, cq.y, cq.z, cq.w};
            float z[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                z[k] = z0[k];
                valid[k] = p0 + k < hw && in_range(z0[k], cfg);
            }
            if (drops) {
                // (row, column) of the four pixels
                int row[4], col[4];
                row[0] = p0 / W;
                col[0] = p0 - row[0] * W;
#pragma unroll
                for (int k = 1; k < 4; ++k) {
                    const bool wrap = col[k - 1] + 1 == W;
                    col[k] = wrap ? 0 : col[k - 1] + 1;
                    row[k] = row[k - 1] + (wrap ? 1 : 0);
                }
                float up[4] = {0.0f, 0.0f, 0.0f, 0.0f}, dn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (rows4) {
                    if (row[0] > 0) {
                        const v4f v = *reinterpret_cast<const v4f *>(img + p0 - W);
                        up[0] = v.x; up[1] = v.y; up[2] = v.z; up[3] = v.w;
                    }
                    if (row[0] < H - 1) {
                        const v4f v = *reinterpret_cast<const v4f *>(img + p0 + W);
                        dn[0] = v.x; dn[1] = v.y; dn[2] = v.z; dn[3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (valid[k] && row[k] > 0) up[k] = img[p0 + k - W];
                        if (valid[k] && row[k] < H - 1) dn[k] = img[p0 + k + W];
                    }
                }
                const float lf = p0 > 0 ? img[p0 - 1] : 0.0f, rt = img[p0 + 4];
                uint32_t w[4];
                philox4x32(c0, A.c1, A.c2, ROVER_DEPTH_SENSOR_STREAM_DROPOUT | (uint32_t)q, A.k0, A.k1, w);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    bool edge = false;
                    if (row[k] > 0) edge |= edge_to(z0[k], up[k], cfg);
                    if (row[k] < H - 1) edge |= edge_to(z0[k], dn[k], cfg);
                    if (col[k] > 0) edge |= edge_to(z0[k], k > 0 ? z0[k - 1] : lf, cfg);
                    if (col[k] < W - 1) edge |= edge_to(z0[k], k < 3 ? z0[k + 1] : rt, cfg);
                    valid[k] = valid[k] && !(unit_uniform(w[k]) < (edge ? cfg.p_edge : cfg.p_drop));
                }
            }
            {
                uint32_t w[4];
                float e[4];
                philox4x32(c0, A.c1, A.c2, ROVER_DEPTH_SENSOR_STREAM_NORMAL | (uint32_t)q, A.k0, A.k1, w);
                box_muller(w[0], w[1], e[0], e[1]);
                box_muller(w[2], w[3], e[2], e[3]);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float t = __fmul_rn(z[k], cfg.sigma2);
                    t = __fadd_rn(t, cfg.sigma1);
                    t = __fmul_rn(z[k], t);
                    const float s = __fadd_rn(t, cfg.sigma0);
                    z[k] = __fadd_rn(z[k], __fmul_rn(s, e[k]));
                }
            }
            if (steps) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float d = cfg.fb / z[k];
                    const float kk = rintf(__fmul_rn(d, cfg.inv_step));
                    valid[k] = valid[k] && kk >= 1.0f;
                    z[k] = cfg.fb / __fmul_rn(kk, cfg.disparity_step);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) z[k] = valid[k] ? z[k] : cfg.invalid_value;
            float *o = dst + p0;
            if (p0 + 3 < hw && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
                v4f v;
                v.x = z[0]; v.y = z[1]; v.z = z[2]; v.w = z[3];
                *reinterpret_cast<v4f *>(o) = v;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (p0 + k < hw) o[k] = z[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) count += __popcll(__ballot(valid[k]));
    }
    if (A.valid_out) {                                              // kernel argument: uniform over the workgroup
        if ((tid & 63) == 0) wave_valid[tid >> 6] = count;
        __syncthreads();
        if (tid == 0) {
            int total = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) total += wave_valid[w];
            A.valid_out[blockIdx.x] = total;
        }
    }
}

int refuse(const char *why) { return rover_internal_fail(ROVER_ERR_INVALID, "rover_depth_sensor_apply: %s", why); }

bool sigma_ok(float v) { return std::isfinite(v) && v >= 0.0f; }
bool prob_ok(float v) { return v >= 0.0f && v <= 1.0f; }     // false for a NaN

}  // namespace

extern "C" {

size_t rover_depth_sensor_cfg_bytes(void) { return sizeof(rover_depth_sensor_cfg); }

int rover_depth_sensor_apply(const rover_depth_sensor_cfg *cfg, const float *src, float *dst, int32_t height, int32_t width,
                             int64_t pitch_floats, int32_t n, uint64_t seed, uint64_t env_id_offset, uint64_t counter,
                             int32_t *valid_out, void *stream)
{
    if (!cfg || !src || !dst) return refuse("NULL argument");
    if (n <= 0) return refuse("n must be > 0");
    if (height <= 0 || width <= 0) return refuse("height and width must be > 0");
    const int64_t hw = (int64_t)height * (int64_t)width;
    if (hw > ROVER_DEPTH_SENSOR_MAX_PIXELS)
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "rover_depth_sensor_apply: %s", "height * width must be <= 16384");
    if (pitch_floats < hw) return refuse("pitch_floats must be >= height * width");
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(valid_out)) & 3)
        return refuse("src, dst and valid_out must be 4-byte aligned");
    if (pitch_floats > (INT64_MAX / 8) / (int64_t)n) return refuse("n * pitch_floats is out of range");
    if (src != dst) {
        const uint64_t bytes = ((uint64_t)(n - 1) * (uint64_t)pitch_floats + (uint64_t)hw) * 4u;
        const uintptr_t a = reinterpret_cast<uintptr_t>(src), b = reinterpret_cast<uintptr_t>(dst);
        if (a < b ? b - a < bytes : a - b < bytes) return refuse("src and dst overlap without being equal");
    }
    const rover_depth_sensor_cfg &c = *cfg;
    if (!sigma_ok(c.sigma0) || !sigma_ok(c.sigma1) || !sigma_ok(c.sigma2)) return refuse("sigma0, sigma1 and sigma2 must be finite and >= 0");
    if (!sigma_ok(c.edge_rel)) return refuse("edge_rel must be finite and >= 0");
    if (!prob_ok(c.p_drop) || !prob_ok(c.p_edge)) return refuse("p_drop and p_edge must be in [0, 1]");
    if (!(c.range_min >= 0.0f)) return refuse("range_min must be >= 0");
    if (!(c.range_max >= c.range_min)) return refuse("range_max must be >= range_min");
    if (!sigma_ok(c.disparity_step)) return refuse("disparity_step must be finite and >= 0");
    if (c.disparity_step > 0.0f) {
        if (!(std::isfinite(c.fb) && c.fb > 0.0f)) return refuse("fb must be finite and > 0 with a disparity step");
        if (!(std::isfinite(c.inv_step) && c.inv_step > 0.0f)) return refuse("inv_step must be finite and > 0 with a disparity step");
    }
    if (c.invalid_value != c.invalid_value) return refuse("invalid_value must not be a NaN");
    int dev;
    if (int rc = device_of(dst, &dev, true)) return rc;
    DeviceGuard guard(dev);
    SensorArgs A;
    A.cfg = c;
    A.src = src;
    A.dst = dst;
    A.valid_out = valid_out;
    A.pitch = (long long)pitch_floats;
    A.id0 = env_id_offset;
    A.height = height;
    A.width = width;
    A.hw = (int)hw;
    A.k0 = (uint32_t)seed; A.k1 = (uint32_t)(seed >> 32);
    A.c1 = (uint32_t)counter; A.c2 = (uint32_t)(counter >> 32);
    hipLaunchKernelGGL(depth_sensor_kernel, dim3((unsigned)n), dim3(TT), 0, static_cast<hipStream_t>(stream), A);
    return launched("depth_sensor_kernel launch: %s");
}

}  // extern "C"
