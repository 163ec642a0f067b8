// scaler_kernels.hip -- skrl's RunningStandardScaler at any width up to 1024 (gfx950 / CDNA4, wave64).
//
// See include/rover_scaler.h for the contract and the reduction order.  Kernels:
//   scaler_partial_kernel<false / true>   one 256-thread workgroup per (chunk of 64 rows, block of 64 columns): lanes run across
//                                         columns (a wave reads 256 contiguous bytes of a row), the four waves take every fourth
//                                         row; float64 sums of x, or of (x - mean)^2, into the workspace;
//   scaler_mean_kernel                    one thread per column: the chunk sums in ascending order -> the batch mean;
//   scaler_merge_kernel                   one workgroup: the chunk sums in ascending order -> the unbiased variance, then skrl's
//                                         _parallel_variance into the block;
//   scaler_apply_kernel                   forward / inverse (+ nan_to_num, + the raw copy) over rows or over rows named by idx:
//                                         a wave per span (one row with idx, 1024 consecutive floats without), moved as a scalar
//                                         head, 16-byte vectors and a scalar tail where the three arrays share their alignment.
// The statistics kernels have *_gated_kernel twins (rover_scaler_train_gated): the same device function behind one load of a gate
// word that no kernel here writes.
// The launch boundary is the only synchronisation between workgroups: no flags, no fences, no atomics.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/rover_hip.h"
#include "../../include/rover_scaler.h"
#include "rover_internal.hpp"
#include "train_math.hpp"   // sanitise

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int MAX_W = ROVER_SCALER_MAX_WIDTH;
constexpr int CH = 64;            // rows per chunk
constexpr int CB = 64;            // columns per workgroup of the partial sums (one wave's lanes)
constexpr int TT = 256;           // threads of the partial-sum, mean and apply kernels
constexpr int SPAN = 1024;        // floats per wave step of the apply kernel without idx (a multiple of 4)
constexpr int APPLY_MAX_BLOCKS = 2048;

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- statistics
template <bool DEV>
__device__ __forceinline__ void scaler_partial_body(const float *x, const int64_t *idx, int rows, int width, const double *mean, double *part)
{
    __shared__ double red[TT / 64][CB];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int c = blockIdx.y * CB + lane;
    const int r0 = blockIdx.x * CH, r1 = min(rows, r0 + CH);
    double s = 0.0;
    if (c < width) {
        const double m = DEV ? mean[c] : 0.0;
        for (int r = r0 + q; r < r1; r += TT / 64) {
            const double v = (double)x[(size_t)(idx ? idx[r] : (int64_t)r) * width + c];
            if (DEV) {
                const double d = v - m;
                s += d * d;
            } else {
                s += v;
            }
        }
    }
    red[q][lane] = s;
    __syncthreads();
    if (q == 0 && c < width) part[(size_t)blockIdx.x * width + c] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}
template <bool DEV>
__global__ __launch_bounds__(TT) void scaler_partial_kernel(const float *x, const int64_t *idx, int rows, int width, const double *mean,
                                                            double *part)
{
    scaler_partial_body<DEV>(x, idx, rows, width, mean, part);
}
template <bool DEV>
__global__ __launch_bounds__(TT) void scaler_partial_gated_kernel(const float *x, const int64_t *idx, int rows, int width,
                                                                  const double *mean, double *part, const int32_t *gate)
{
    if (*gate) return;
    scaler_partial_body<DEV>(x, idx, rows, width, mean, part);
}

__device__ __forceinline__ void scaler_mean_body(const double *part, int n_chunks, int rows, int width, double *mean)
{
    const int c = blockIdx.x * TT + threadIdx.x;
    if (c >= width) return;
    double s = 0.0;
    for (int k = 0; k < n_chunks; ++k) s += part[(size_t)k * width + c];
    mean[c] = s / (double)rows;
}
__global__ __launch_bounds__(TT) void scaler_mean_kernel(const double *part, int n_chunks, int rows, int width, double *mean)
{
    scaler_mean_body(part, n_chunks, rows, width, mean);
}
__global__ __launch_bounds__(TT) void scaler_mean_gated_kernel(const double *part, int n_chunks, int rows, int width, double *mean,
                                                               const int32_t *gate)
{
    if (*gate) return;
    scaler_mean_body(part, n_chunks, rows, width, mean);
}

__device__ __forceinline__ void scaler_merge_body(double *scaler, int width, int rows, const double *bmean, const double *part, int n_chunks)
{
    const int c = threadIdx.x;
    double *mean = scaler, *var = scaler + width;
    const double cnt = scaler[2 * width], bc = (double)rows, tot = cnt + bc;
    if (c < width) {
        double m2b = 0.0;
        for (int k = 0; k < n_chunks; ++k) m2b += part[(size_t)k * width + c];
        const double bvar = m2b / (double)(rows - 1);                                 // torch.var: unbiased
        const double delta = bmean[c] - mean[c];
        const double m2 = var[c] * cnt + bvar * bc + delta * delta * cnt * bc / tot;  // skrl _parallel_variance
        mean[c] = mean[c] + delta * bc / tot;
        var[c] = m2 / tot;
    }
    __syncthreads();   // every column has read the old count
    if (c == 0) scaler[2 * width] = tot;
}
__global__ __launch_bounds__(MAX_W) void scaler_merge_kernel(double *scaler, int width, int rows, const double *bmean, const double *part,
                                                             int n_chunks)
{
    scaler_merge_body(scaler, width, rows, bmean, part, n_chunks);
}
__global__ __launch_bounds__(MAX_W) void scaler_merge_gated_kernel(double *scaler, int width, int rows, const double *bmean,
                                                                   const double *part, int n_chunks, const int32_t *gate)
{
    if (*gate) return;
    scaler_merge_body(scaler, width, rows, bmean, part, n_chunks);
}

// ---- transform
__device__ __forceinline__ float clampf_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }   // NaN passes

struct ApplyArgs {
    const double *scaler;
    const float *x;
    const int64_t *idx;
    float *out, *raw;
    long long n_spans;
    size_t total;                 // rows * width
    int width, inverse, sanitise, vec;
    float eps, clip;
};

__global__ __launch_bounds__(TT) void scaler_apply_kernel(ApplyArgs A)
{
    // per column: (float)mean and sqrtf((float)var) (+ eps for the forward transform): the operands of rover_scaler.h's expressions
    __shared__ float s_mu[MAX_W], s_sd[MAX_W];
    const int w = A.width;
    for (int c = threadIdx.x; c < w; c += TT) {
        s_mu[c] = (float)A.scaler[c];
        const float sd = sqrtf((float)A.scaler[w + c]);
        s_sd[c] = A.inverse ? sd : __fadd_rn(sd, A.eps);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float clip = A.clip;
    const bool inverse = A.inverse != 0, san = A.sanitise != 0;
    auto clean = [&](float v) { return san ? sanitise(v) : v; };
    auto map = [&](float v, int c) {
        return inverse ? __fadd_rn(__fmul_rn(s_sd[c], clampf_nan(v, -clip, clip)), s_mu[c])
                       : clampf_nan(__fdiv_rn(__fsub_rn(v, s_mu[c]), s_sd[c]), -clip, clip);
    };
    for (long long sp = (long long)blockIdx.x * (TT / 64) + wave; sp < A.n_spans; sp += (long long)gridDim.x * (TT / 64)) {
        size_t start;
        int len, col0;
        if (A.idx) {
            start = (size_t)A.idx[sp] * w; len = w; col0 = 0;
        } else {
            start = (size_t)sp * SPAN;
            len = (int)min((size_t)SPAN, A.total - start);
            col0 = (int)(start % (size_t)w);
        }
        const float *xs = A.x + start;
        float *os = A.out + start;
        float *rs = A.raw ? A.raw + start : nullptr;
        // scalar head up to the 16-byte boundary (the whole span when the arrays do not share their alignment), vectors, scalar tail
        const int head = A.vec ? min(len, (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(xs) >> 2) & 3u)) & 3u)) : len;
        const int nv = (len - head) >> 2;
        const int tail0 = head + 4 * nv;
        auto one = [&](int k) {
            const float v = clean(xs[k]);
            if (rs) rs[k] = v;
            os[k] = map(v, (col0 + k) % w);
        };
        for (int k = lane; k < head; k += 64) one(k);
        for (int k = tail0 + lane; k < len; k += 64) one(k);
        for (int j = lane; j < nv; j += 64) {
            const int k = head + 4 * j;
            v4f v = *reinterpret_cast<const v4f *>(xs + k);
            v.x = clean(v.x); v.y = clean(v.y); v.z = clean(v.z); v.w = clean(v.w);
            if (rs) *reinterpret_cast<v4f *>(rs + k) = v;
            int c = (col0 + k) % w;
            v4f o;
            o.x = map(v.x, c); c = c + 1 == w ? 0 : c + 1;
            o.y = map(v.y, c); c = c + 1 == w ? 0 : c + 1;
            o.z = map(v.z, c); c = c + 1 == w ? 0 : c + 1;
            o.w = map(v.w, c);
            *reinterpret_cast<v4f *>(os + k) = o;
        }
    }
}

bool width_ok(int32_t width) { return width >= 1 && width <= MAX_W; }
size_t ws_doubles(int width, int rows) { return (size_t)width * (1 + (size_t)cdiv(rows, CH)); }

}  // namespace

extern "C" {

int rover_scaler_default_hparams(rover_scaler_hparams *h)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "hparams is NULL");
    h->eps = 1e-8f;
    h->clip = 5.0f;
    return ROVER_OK;
}
size_t rover_scaler_hparams_bytes(void) { return sizeof(rover_scaler_hparams); }
size_t rover_scaler_doubles(int32_t width) { return width_ok(width) ? 2 * (size_t)width + 1 : 0; }
size_t rover_scaler_workspace_bytes(int32_t width, int32_t max_rows)
{
    return width_ok(width) && max_rows >= 2 ? sizeof(double) * ws_doubles(width, max_rows) : 0;
}

}  // extern "C"

namespace {

// rover_scaler_train (gate == NULL: the ungated kernels, the launches as they always were) and rover_scaler_train_gated
int train_impl(const rover_scaler_hparams *h, double *scaler, int32_t width, const float *x, const int64_t *idx, int32_t rows, void *ws,
               size_t ws_bytes, const int32_t *gate, void *stream)
{
    if (!h || !scaler || !x || !ws) return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_train: NULL argument");
    if (!width_ok(width)) return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_train: width must be in [1, 1024]");
    if (rows < 2) return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_train: rows must be >= 2");
    if (ws_bytes < rover_scaler_workspace_bytes(width, rows))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_train: workspace too small");
    if ((reinterpret_cast<uintptr_t>(scaler) | reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(idx)) & 7)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_train: scaler, ws and idx must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(x) & 3) return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_train: x must be 4-byte aligned");
    int dev;
    if (int rc = device_of(scaler, &dev, true)) return rc;
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *bmean = static_cast<double *>(ws), *part = bmean + width;
    const int n_chunks = cdiv(rows, CH);
    const dim3 grid((unsigned)n_chunks, (unsigned)cdiv(width, CB));
    if (gate) {
        hipLaunchKernelGGL(scaler_partial_gated_kernel<false>, grid, dim3(TT), 0, s, x, idx, (int)rows, (int)width, (const double *)nullptr,
                           part, gate);
        if (int rc = launched("scaler_partial_kernel launch: %s")) return rc;
        hipLaunchKernelGGL(scaler_mean_gated_kernel, dim3(cdiv(width, TT)), dim3(TT), 0, s, (const double *)part, n_chunks, (int)rows,
                           (int)width, bmean, gate);
        if (int rc = launched("scaler_mean_kernel launch: %s")) return rc;
        hipLaunchKernelGGL(scaler_partial_gated_kernel<true>, grid, dim3(TT), 0, s, x, idx, (int)rows, (int)width, (const double *)bmean,
                           part, gate);
        if (int rc = launched("scaler_partial_kernel launch: %s")) return rc;
        hipLaunchKernelGGL(scaler_merge_gated_kernel, dim3(1), dim3(MAX_W), 0, s, scaler, (int)width, (int)rows, (const double *)bmean,
                           (const double *)part, n_chunks, gate);
        return launched("scaler_merge_kernel launch: %s");
    }
    hipLaunchKernelGGL(scaler_partial_kernel<false>, grid, dim3(TT), 0, s, x, idx, (int)rows, (int)width, (const double *)nullptr, part);
    if (int rc = launched("scaler_partial_kernel launch: %s")) return rc;
    hipLaunchKernelGGL(scaler_mean_kernel, dim3(cdiv(width, TT)), dim3(TT), 0, s, (const double *)part, n_chunks, (int)rows, (int)width,
                       bmean);
    if (int rc = launched("scaler_mean_kernel launch: %s")) return rc;
    hipLaunchKernelGGL(scaler_partial_kernel<true>, grid, dim3(TT), 0, s, x, idx, (int)rows, (int)width, (const double *)bmean, part);
    if (int rc = launched("scaler_partial_kernel launch: %s")) return rc;
    hipLaunchKernelGGL(scaler_merge_kernel, dim3(1), dim3(MAX_W), 0, s, scaler, (int)width, (int)rows, (const double *)bmean,
                       (const double *)part, n_chunks);
    return launched("scaler_merge_kernel launch: %s");
}

}  // namespace

extern "C" {

int rover_scaler_train(const rover_scaler_hparams *h, double *scaler, int32_t width, const float *x, const int64_t *idx, int32_t rows,
                       void *ws, size_t ws_bytes, void *stream)
{
    return train_impl(h, scaler, width, x, idx, rows, ws, ws_bytes, nullptr, stream);
}

int rover_scaler_train_gated(const rover_scaler_hparams *h, double *scaler, int32_t width, const float *x, const int64_t *idx,
                             int32_t rows, void *ws, size_t ws_bytes, const int32_t *gate, void *stream)
{
    if (!gate) return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_train_gated: gate is NULL");
    if (reinterpret_cast<uintptr_t>(gate) & 3) return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_train_gated: gate must be 4-byte aligned");
    return train_impl(h, scaler, width, x, idx, rows, ws, ws_bytes, gate, stream);
}

int rover_scaler_apply(const rover_scaler_hparams *h, const double *scaler, int32_t width, const float *x, const int64_t *idx,
                       int32_t rows, int32_t flags, float *out, float *raw_out, void *stream)
{
    if (!h || !scaler || !x || !out) return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_apply: NULL argument");
    if (!width_ok(width)) return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_apply: width must be in [1, 1024]");
    if (rows < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_apply: rows must be >= 1");
    if (flags & ~(ROVER_SCALER_INVERSE | ROVER_SCALER_SANITISE))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_apply: unknown flag");
    if (raw_out && (raw_out == x || raw_out == out))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_apply: raw_out must not alias x or out");
    if ((reinterpret_cast<uintptr_t>(scaler) | reinterpret_cast<uintptr_t>(idx)) & 7)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_apply: scaler and idx must be 8-byte aligned");
    const uintptr_t px = reinterpret_cast<uintptr_t>(x), po = reinterpret_cast<uintptr_t>(out), pr = reinterpret_cast<uintptr_t>(raw_out);
    if ((px | po | pr) & 3) return rover_internal_fail(ROVER_ERR_INVALID, "rover_scaler_apply: x, out and raw_out must be 4-byte aligned");
    int dev;
    if (int rc = device_of(scaler, &dev, true)) return rc;
    DeviceGuard guard(dev);
    ApplyArgs A;
    A.scaler = scaler; A.x = x; A.idx = idx; A.out = out; A.raw = raw_out;
    A.total = (size_t)rows * (size_t)width;
    A.n_spans = idx ? (long long)rows : (long long)((A.total + SPAN - 1) / SPAN);
    A.width = width;
    A.inverse = (flags & ROVER_SCALER_INVERSE) != 0;
    A.sanitise = (flags & ROVER_SCALER_SANITISE) != 0;
    A.vec = ((px ^ po) & 15) == 0 && (!raw_out || ((px ^ pr) & 15) == 0);
    A.eps = h->eps; A.clip = h->clip;
    const long long blocks = (A.n_spans + TT / 64 - 1) / (TT / 64);
    hipLaunchKernelGGL(scaler_apply_kernel, dim3((unsigned)(blocks < APPLY_MAX_BLOCKS ? blocks : APPLY_MAX_BLOCKS)), dim3(TT), 0,
                       static_cast<hipStream_t>(stream), A);
    return launched("scaler_apply_kernel launch: %s");
}

}  // extern "C"
