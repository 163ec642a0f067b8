// tracker_kernels.hip -- skrl's reward / episode tracking on the device (gfx950 / CDNA4, wave64).
//
// See include/rover_tracker.h for the contract, the state layout and the reduction orders.  Kernels:
//   tracker_init_kernel       the initial state;
//   tracker_accum_kernel      one 256-thread workgroup per chunk of 256 envs: cum_r += r, cum_t += 1, the chunk's count of finished
//                             envs (ballot + popcount per wave, LDS across the four waves) and its max / min / float64 sum (LDS
//                             tree) into the workspace;
//   tracker_commit_kernel     one workgroup: the chunk results combined in a fixed order, the finished envs of the chunks that
//                             have any appended to the two windows in env-id order (a running count across the chunks, LDS across
//                             the waves, ballot + popcount inside a wave: csrc/trace_kernels.hip's commit kernel), cum_r / cum_t
//                             zeroed there, the windows' statistics, the accumulators;
//   tracker_track_kernel      one thread per value into its slot;
//   tracker_snapshot_kernel   the accumulators and the slots copied out, then cleared.
// The launch boundary is the only synchronisation between workgroups: no flags, no fences, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/rover_hip.h"
#include "../../include/rover_tracker.h"
#include "rover_internal.hpp"

namespace {

constexpr int WIN = ROVER_TRACKER_WINDOW;
constexpr int TT = ROVER_TRACKER_CHUNK;
constexpr int HDR = ROVER_TRACKER_HDR_WORDS;
constexpr int ACC = ROVER_TRACKER_ACC_WORDS;
constexpr int MAX_SLOTS = ROVER_TRACKER_MAX_SLOTS;
// header words
constexpr int W_N = 0, W_SLOTS = 1, W_HEAD = 2, W_LEN = 3, W_STEPS = 4, W_WSTEPS = 5;
constexpr int W_SUM = 8, W_MAX = 14, W_MIN = 17, W_RING_R = 20, W_RING_T = 120;

__host__ __device__ inline int cdiv(int a, int b) { return (int)(((long long)a + b - 1) / b); }
__host__ __device__ inline size_t cum_word(int slots) { return (size_t)HDR + 6 * (size_t)slots; }

__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (a > b ? a : b); }
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (a < b ? a : b); }

struct Slots {
    double *sum;
    long long *count;
    float *mx, *mn;
};
__device__ __forceinline__ Slots slots_of(int32_t *state, int slots)
{
    Slots s;
    s.sum = reinterpret_cast<double *>(state + HDR);
    s.count = reinterpret_cast<long long *>(state + HDR + 2 * (size_t)slots);
    s.mx = reinterpret_cast<float *>(state + HDR + 4 * (size_t)slots);
    s.mn = s.mx + slots;
    return s;
}

// x[t] = op(x[t], x[t + s]) for s = 128 ... 1 over the three LDS arrays; the results are at [0] behind the last barrier
__device__ __forceinline__ void tree(double *s_sum, float *s_max, float *s_min, int t)
{
    for (int s = TT / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) {
            s_sum[t] = s_sum[t] + s_sum[t + s];
            s_max[t] = max_nan(s_max[t], s_max[t + s]);
            s_min[t] = min_nan(s_min[t], s_min[t + s]);
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(TT) void tracker_init_kernel(int32_t *state, int n, int slots, size_t words)
{
    float *f = reinterpret_cast<float *>(state);
    const size_t mx0 = (size_t)HDR + 4 * (size_t)slots, mn0 = mx0 + slots, cum0 = mn0 + slots;
    for (size_t w = (size_t)blockIdx.x * TT + threadIdx.x; w < words; w += (size_t)gridDim.x * TT) {
        if (w == W_N) state[w] = n;
        else if (w == W_SLOTS) state[w] = slots;
        else if ((w >= W_MAX && w < W_MIN) || (w >= mx0 && w < mn0)) f[w] = -INFINITY;
        else if ((w >= W_MIN && w < W_RING_R) || (w >= mn0 && w < cum0)) f[w] = INFINITY;
        else state[w] = 0;
    }
}

// the flags as the collectors hold them (float32: terminated + truncated != 0, skrl's expression) or as the envs return them (bytes)
__device__ __forceinline__ bool finished(const float *term, const float *trunc, int e)
{
    return (trunc ? __fadd_rn(term[e], trunc[e]) : term[e]) != 0.0f;
}
__device__ __forceinline__ bool finished(const uint8_t *term, const uint8_t *trunc, int e)
{
    return (term[e] | (trunc ? trunc[e] : (uint8_t)0)) != 0;
}

template <typename F>
__global__ __launch_bounds__(TT) void tracker_accum_kernel(int32_t *state, int n, int slots, const float *__restrict__ rew,
                                                           const F *__restrict__ term, const F *__restrict__ trunc,
                                                           double *psum, float *pmax, float *pmin, int32_t *pcount)
{
    __shared__ double s_sum[TT];
    __shared__ float s_max[TT], s_min[TT];
    __shared__ int s_cnt[TT / 64];
    const int t = threadIdx.x, e = blockIdx.x * TT + t;
    float *cum_r = reinterpret_cast<float *>(state + cum_word(slots));
    int32_t *cum_t = reinterpret_cast<int32_t *>(cum_r + n);
    double v = 0.0;
    float mx = -INFINITY, mn = INFINITY;
    bool fin = false;
    if (e < n) {
        const float r = rew[e];
        cum_r[e] = __fadd_rn(cum_r[e], r);
        cum_t[e] = cum_t[e] + 1;
        fin = finished(term, trunc, e);
        v = (double)r;
        mx = mn = r;
    }
    const unsigned long long ballot = __ballot(fin);
    if ((t & 63) == 0) s_cnt[t >> 6] = __popcll(ballot);
    s_sum[t] = v; s_max[t] = mx; s_min[t] = mn;
    tree(s_sum, s_max, s_min, t);
    if (t == 0) {
        psum[blockIdx.x] = s_sum[0];
        pmax[blockIdx.x] = s_max[0];
        pmin[blockIdx.x] = s_min[0];
        pcount[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    }
}

template <typename F>
__global__ __launch_bounds__(TT) void tracker_commit_kernel(int32_t *state, int n, int slots, const F *__restrict__ term,
                                                            const F *__restrict__ trunc, const double *__restrict__ psum,
                                                            const float *__restrict__ pmax, const float *__restrict__ pmin,
                                                            const int32_t *__restrict__ pcount, int nb)
{
    __shared__ double s_sum[TT];
    __shared__ float s_max[TT], s_min[TT];
    __shared__ int s_k[TT], s_cnt[TT / 64];
    __shared__ float s_wr[WIN];
    __shared__ int s_wt[WIN];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float *cum_r = reinterpret_cast<float *>(state + cum_word(slots));
    int32_t *cum_t = reinterpret_cast<int32_t *>(cum_r + n);
    float *ring_r = reinterpret_cast<float *>(state + W_RING_R);
    int32_t *ring_t = state + W_RING_T;
    // thread 0 writes them behind the barriers below; brought into range so that a block nobody initialised cannot index past a ring
    const int head = (state[W_HEAD] % WIN + WIN) % WIN, len = min(max(state[W_LEN], 0), WIN);

    // the step's instantaneous max / min / sum and the count K of finished envs
    double v = 0.0;
    float mx = -INFINITY, mn = INFINITY;
    int k = 0;
    for (int b = t; b < nb; b += TT) {
        v = v + psum[b];
        mx = max_nan(mx, pmax[b]);
        mn = min_nan(mn, pmin[b]);
        k += pcount[b];
    }
    s_sum[t] = v; s_max[t] = mx; s_min[t] = mn; s_k[t] = k;
    for (int s = TT / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) {
            s_sum[t] = s_sum[t] + s_sum[t + s];
            s_max[t] = max_nan(s_max[t], s_max[t + s]);
            s_min[t] = min_nan(s_min[t], s_min[t + s]);
            s_k[t] += s_k[t + s];
        }
    }
    __syncthreads();
    const int K = s_k[0];

    // the finished envs into the windows, in env-id order; every branch on pcount[b] is uniform over the workgroup
    if (K > 0) {
        int off = 0;
        for (int b = 0; b < nb; ++b) {
            const int c = pcount[b];
            if (c == 0) continue;
            const int e = b * TT + t;
            bool fin = false;
            if (e < n) fin = finished(term, trunc, e);
            const unsigned long long ballot = __ballot(fin);
            if (lane == 0) s_cnt[wave] = __popcll(ballot);
            __syncthreads();
            int w_off = 0;
#pragma unroll
            for (int w = 0; w < TT / 64; ++w)
                if (w < wave) w_off += s_cnt[w];
            if (fin) {
                const int rank = off + w_off + __popcll(ballot & ((1ull << lane) - 1ull));
                if (rank >= K - WIN) {
                    const int slot = (int)(((long long)head + rank) % WIN);
                    ring_r[slot] = cum_r[e];
                    ring_t[slot] = cum_t[e];
                }
                cum_r[e] = 0.0f;
                cum_t[e] = 0;
            }
            off += c;
            __syncthreads();                                 // s_cnt is rewritten by the next chunk
        }
    }
    const int new_head = (int)(((long long)head + K) % WIN);
    const int new_len = (int)min((long long)WIN, (long long)len + K);
    __syncthreads();                                         // the ring entries written above are visible to this workgroup
    if (t < new_len) {                                       // oldest to newest
        const int slot = ((new_head - new_len + t) % WIN + WIN) % WIN;
        s_wr[t] = ring_r[slot];
        s_wt[t] = ring_t[slot];
    }
    __syncthreads();
    if (t != 0) return;
    double *acc_sum = reinterpret_cast<double *>(state + W_SUM);
    float *acc_max = reinterpret_cast<float *>(state + W_MAX), *acc_min = reinterpret_cast<float *>(state + W_MIN);
    state[W_HEAD] = new_head;
    state[W_LEN] = new_len;
    state[W_STEPS] = state[W_STEPS] + 1;
    acc_sum[0] = acc_sum[0] + (double)(float)(s_sum[0] / (double)n);
    acc_max[0] = max_nan(acc_max[0], s_max[0]);
    acc_min[0] = min_nan(acc_min[0], s_min[0]);
    if (new_len > 0) {
        double sr = 0.0, st = 0.0;
        float rmx = -INFINITY, rmn = INFINITY, tmx = -INFINITY, tmn = INFINITY;
        for (int i = 0; i < new_len; ++i) {
            const float r = s_wr[i], tt = (float)s_wt[i];
            sr = sr + (double)r;
            st = st + (double)s_wt[i];
            rmx = max_nan(rmx, r); rmn = min_nan(rmn, r);
            tmx = max_nan(tmx, tt); tmn = min_nan(tmn, tt);
        }
        state[W_WSTEPS] = state[W_WSTEPS] + 1;
        acc_sum[1] = acc_sum[1] + sr / (double)new_len;
        acc_sum[2] = acc_sum[2] + st / (double)new_len;
        acc_max[1] = max_nan(acc_max[1], rmx); acc_min[1] = min_nan(acc_min[1], rmn);
        acc_max[2] = max_nan(acc_max[2], tmx); acc_min[2] = min_nan(acc_min[2], tmn);
    }
}

__global__ __launch_bounds__(TT) void tracker_track_kernel(int32_t *state, int slots, int first, const float *__restrict__ values,
                                                           int count)
{
    const int i = blockIdx.x * TT + threadIdx.x;
    if (i >= count) return;
    const Slots s = slots_of(state, slots);
    const int k = first + i;
    const float v = values[i];
    s.sum[k] = s.sum[k] + (double)v;
    s.count[k] = s.count[k] + 1;
    s.mx[k] = max_nan(s.mx[k], v);
    s.mn[k] = min_nan(s.mn[k], v);
}

__global__ __launch_bounds__(TT) void tracker_snapshot_kernel(int32_t *state, int slots, int32_t *out, int clear_window)
{
    float *f = reinterpret_cast<float *>(state);
    const int words = ACC + 6 * slots;
    const int mx0 = ACC + 4 * slots, mn0 = mx0 + slots;
    for (int w = threadIdx.x; w < words; w += TT) {
        const size_t src = w < ACC ? (size_t)w : (size_t)HDR + (w - ACC);
        out[w] = state[src];
        if (w == W_N || w == W_SLOTS) continue;
        if (w == W_HEAD || w == W_LEN) {
            if (clear_window) state[src] = 0;
        } else if ((w >= W_MAX && w < W_MIN) || (w >= mx0 && w < mn0)) {
            f[src] = -INFINITY;
        } else if ((w >= W_MIN && w < ACC) || w >= mn0) {
            f[src] = INFINITY;
        } else {
            state[src] = 0;
        }
    }
}

bool slots_ok(int32_t slots) { return slots >= 0 && slots <= MAX_SLOTS; }
int check_state(const char *who, const void *state, int32_t n, int32_t slots)
{
    if (!state) return rover_internal_fail(ROVER_ERR_INVALID, "%s: state is NULL", who);
    if (n < 1) return rover_internal_fail(ROVER_ERR_INVALID, "%s: n must be >= 1", who);
    if (!slots_ok(slots)) return rover_internal_fail(ROVER_ERR_INVALID, "%s: slots must be in [0, 4096]", who);
    if (reinterpret_cast<uintptr_t>(state) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "%s: state must be 8-byte aligned", who);
    return ROVER_OK;
}

}  // namespace

extern "C" {

size_t rover_tracker_state_bytes(int32_t n, int32_t slots)
{
    if (n < 1 || !slots_ok(slots)) return 0;
    return (4 * (cum_word(slots) + 2 * (size_t)n) + 7) & ~(size_t)7;
}
size_t rover_tracker_workspace_bytes(int32_t n) { return n < 1 ? 0 : (20 * (size_t)cdiv(n, TT) + 7) & ~(size_t)7; }
size_t rover_tracker_snapshot_words(int32_t slots) { return slots_ok(slots) ? (size_t)ACC + 6 * (size_t)slots : 0; }

int rover_tracker_init(void *state, int32_t n, int32_t slots, void *stream)
{
    if (int rc = check_state("rover_tracker_init", state, n, slots)) return rc;
    int dev;
    if (int rc = device_of(state, &dev, true)) return rc;
    DeviceGuard guard(dev);
    const size_t words = rover_tracker_state_bytes(n, slots) / 4;
    const size_t blocks = (words + TT - 1) / TT;
    hipLaunchKernelGGL(tracker_init_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(TT), 0, static_cast<hipStream_t>(stream),
                       static_cast<int32_t *>(state), (int)n, (int)slots, words);
    return launched("tracker_init_kernel launch: %s");
}

int rover_tracker_step(void *state, int32_t n, int32_t slots, const float *rew, const void *terminated, const void *truncated,
                       int32_t flag_bytes, void *ws, size_t ws_bytes, void *stream)
{
    if (int rc = check_state("rover_tracker_step", state, n, slots)) return rc;
    if (!rew || !terminated || !ws) return rover_internal_fail(ROVER_ERR_INVALID, "rover_tracker_step: NULL argument");
    if (ws_bytes < rover_tracker_workspace_bytes(n)) return rover_internal_fail(ROVER_ERR_INVALID, "rover_tracker_step: workspace too small");
    if (reinterpret_cast<uintptr_t>(ws) & 7) return rover_internal_fail(ROVER_ERR_INVALID, "rover_tracker_step: ws must be 8-byte aligned");
    if (flag_bytes != 4 && flag_bytes != 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_tracker_step: flag_bytes must be 4 or 1");
    if ((reinterpret_cast<uintptr_t>(rew) & 3) ||
        (flag_bytes == 4 && ((reinterpret_cast<uintptr_t>(terminated) | reinterpret_cast<uintptr_t>(truncated)) & 3)))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_tracker_step: rew and float32 flags must be 4-byte aligned");
    int dev;
    if (int rc = device_of(state, &dev, true)) return rc;
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = cdiv(n, TT);
    double *psum = static_cast<double *>(ws);
    float *pmax = reinterpret_cast<float *>(psum + nb), *pmin = pmax + nb;
    int32_t *pcount = reinterpret_cast<int32_t *>(pmin + nb);
    int32_t *st = static_cast<int32_t *>(state);
    if (flag_bytes == 4) {
        const float *te = static_cast<const float *>(terminated), *tr = static_cast<const float *>(truncated);
        hipLaunchKernelGGL(tracker_accum_kernel<float>, dim3((unsigned)nb), dim3(TT), 0, s, st, (int)n, (int)slots, rew, te, tr, psum, pmax,
                           pmin, pcount);
        if (int rc = launched("tracker_accum_kernel launch: %s")) return rc;
        hipLaunchKernelGGL(tracker_commit_kernel<float>, dim3(1), dim3(TT), 0, s, st, (int)n, (int)slots, te, tr, (const double *)psum,
                           (const float *)pmax, (const float *)pmin, (const int32_t *)pcount, nb);
    } else {
        const uint8_t *te = static_cast<const uint8_t *>(terminated), *tr = static_cast<const uint8_t *>(truncated);
        hipLaunchKernelGGL(tracker_accum_kernel<uint8_t>, dim3((unsigned)nb), dim3(TT), 0, s, st, (int)n, (int)slots, rew, te, tr, psum,
                           pmax, pmin, pcount);
        if (int rc = launched("tracker_accum_kernel launch: %s")) return rc;
        hipLaunchKernelGGL(tracker_commit_kernel<uint8_t>, dim3(1), dim3(TT), 0, s, st, (int)n, (int)slots, te, tr, (const double *)psum,
                           (const float *)pmax, (const float *)pmin, (const int32_t *)pcount, nb);
    }
    return launched("tracker_commit_kernel launch: %s");
}

int rover_tracker_track(void *state, int32_t n, int32_t slots, int32_t first_slot, const float *values, int32_t count, void *stream)
{
    if (int rc = check_state("rover_tracker_track", state, n, slots)) return rc;
    if (!values || (reinterpret_cast<uintptr_t>(values) & 3))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_tracker_track: values must be a 4-byte aligned device pointer");
    if (first_slot < 0 || count < 1 || (long long)first_slot + count > slots)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_tracker_track: slot out of range");
    int dev;
    if (int rc = device_of(state, &dev, true)) return rc;
    DeviceGuard guard(dev);
    hipLaunchKernelGGL(tracker_track_kernel, dim3((unsigned)cdiv(count, TT)), dim3(TT), 0, static_cast<hipStream_t>(stream),
                       static_cast<int32_t *>(state), (int)slots, (int)first_slot, values, (int)count);
    return launched("tracker_track_kernel launch: %s");
}

int rover_tracker_snapshot(void *state, int32_t n, int32_t slots, void *out, int32_t clear_window, void *stream)
{
    if (int rc = check_state("rover_tracker_snapshot", state, n, slots)) return rc;
    if (!out || (reinterpret_cast<uintptr_t>(out) & 7))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_tracker_snapshot: out must be an 8-byte aligned pointer");
    int dev;
    if (int rc = device_of(state, &dev, true)) return rc;
    DeviceGuard guard(dev);
    hipLaunchKernelGGL(tracker_snapshot_kernel, dim3(1), dim3(TT), 0, static_cast<hipStream_t>(stream), static_cast<int32_t *>(state),
                       (int)slots, static_cast<int32_t *>(out), (int)(clear_window != 0));
    return launched("tracker_snapshot_kernel launch: %s");
}

}  // extern "C"
