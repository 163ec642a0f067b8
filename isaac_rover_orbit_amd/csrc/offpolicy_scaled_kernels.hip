// offpolicy_scaled_kernels.hip -- the path between the replay ring and a TD3 / SAC update behind skrl's RunningStandardScaler
// (gfx950 / CDNA4, wave64).
//
// See include/rover_offpolicy_scaled.h for the contract.  Kernels:
//   offpolicy_stage_resolve_kernel   one thread per sampled index: offpolicy_net.hpp's gather rules (row 0 and a sticky bad_index word
//                                    for an index or a ring position out of range), the two ring-row lists as int64 and the
//                                    compact transition (actions, reward, terminated byte);
//   offpolicy_stage_rows_kernel      one wave per destination row: out[i] = forward(x[src[i]]) with scaler_kernels.hip's forward
//                                    expression.  The destination decides the split: a dword head up to its 16-byte boundary,
//                                    16-byte stores, a dword tail.  The 16-byte loads that feed them are dword-aligned only (global
//                                    memory takes a 16-byte load at any dword address): a 965-float row is 3860 bytes, so a source
//                                    row shares its destination's phase for one index in four and an "only where the phases
//                                    agree" rule would move three rows in four dword by dword.
// No flags, no fences, no atomics; the launch boundary orders the two kernels and the scaler's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/rover_hip.h"
#include "../../include/rover_offpolicy_scaled.h"
#include "rover_internal.hpp"
#include "train_shared.hpp"   // cdiv, v4f

namespace {

constexpr int MAX_W = ROVER_SCALER_MAX_WIDTH;
constexpr int TT = 256;                   // threads of both kernels
constexpr int WAVES = TT / 64;
constexpr int ROWS_MAX_BLOCKS = 512;      // the per-column table is built once per workgroup: at the reference's batch 8 rows share it
constexpr int MAX_ACT = 16;

typedef float v4f_u __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte load at a dword address

// ---- resolve
struct ResolveArgs {
    const int64_t *idx; int n; int64_t valid;
    int num_envs, slots, act_dim;
    const int32_t *pos;
    const float *act, *rew; const uint8_t *term;
    int64_t *rows_s, *rows_n;
    float *a, *r; uint8_t *t;
    int32_t *bad;
};
__global__ __launch_bounds__(TT) void offpolicy_stage_resolve_kernel(ResolveArgs A)
{
    const int row = blockIdx.x * TT + threadIdx.x;
    if (row >= A.n) return;
    int64_t i = A.idx[row];
    bool bad = i < 0 || i >= A.valid;
    if (bad) i = 0;
    const int64_t k = i / A.num_envs, e = i - k * A.num_envs;
    int32_t p = A.pos[k];
    if (p < 0 || p >= A.slots) { bad = true; p = 0; }
    if (bad) *A.bad = 1;                                  // every writer stores the same word
    A.rows_s[row] = (int64_t)p * A.num_envs + e;
    A.rows_n[row] = (int64_t)(p + 1 == A.slots ? 0 : p + 1) * A.num_envs + e;
    for (int c = 0; c < A.act_dim; ++c) A.a[(size_t)row * A.act_dim + c] = A.act[(size_t)i * A.act_dim + c];
    A.r[row] = A.rew[i];
    A.t[row] = A.term[i];
}

// ---- stage
__device__ __forceinline__ float clampf_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }   // NaN passes

struct RowsArgs {
    const double *scaler;
    const float *x; int64_t x_rows;
    const int64_t *src; int n;
    float *out;
    int32_t *bad;
    int width;
    float eps, clip;
};
__global__ __launch_bounds__(TT) void offpolicy_stage_rows_kernel(RowsArgs A)
{
    // per column: (float)mean and sqrtf((float)var) + eps, the operands of rover_scaler.h's forward expression
    __shared__ float s_mu[MAX_W], s_sd[MAX_W];
    const int w = A.width;
    for (int c = threadIdx.x; c < w; c += TT) {
        s_mu[c] = (float)A.scaler[c];
        s_sd[c] = __fadd_rn(sqrtf((float)A.scaler[w + c]), A.eps);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float clip = A.clip;
    auto map = [&](float v, int c) { return clampf_nan(__fdiv_rn(__fsub_rn(v, s_mu[c]), s_sd[c]), -clip, clip); };
    for (int i = blockIdx.x * WAVES + wave; i < A.n; i += gridDim.x * WAVES) {
        int64_t s = A.src[i];
        if (s < 0 || s >= A.x_rows) {
            s = 0;
            if (A.bad && lane == 0) *A.bad = 1;
        }
        const float *xs = A.x + (size_t)s * w;
        float *os = A.out + (size_t)i * w;
        const int head = min(w, (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(os) >> 2) & 3u)) & 3u));
        const int nv = (w - head) >> 2;
        const int tail0 = head + 4 * nv;
        for (int k = lane; k < head; k += 64) os[k] = map(xs[k], k);
        for (int k = tail0 + lane; k < w; k += 64) os[k] = map(xs[k], k);
        for (int j = lane; j < nv; j += 64) {
            const int k = head + 4 * j;
            const v4f_u v = *reinterpret_cast<const v4f_u *>(xs + k);
            v4f o;
            o.x = map(v.x, k);
            o.y = map(v.y, k + 1);
            o.z = map(v.z, k + 2);
            o.w = map(v.w, k + 3);
            *reinterpret_cast<v4f *>(os + k) = o;
        }
    }
}

bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

int rover_offpolicy_stage_resolve(const int64_t *idx, int32_t n, int64_t valid_rows, int32_t num_envs, int32_t slots,
                                  const int32_t *ring_pos, const float *actions, int32_t act_dim, const float *rewards,
                                  const uint8_t *terminated, int64_t *rows_s, int64_t *rows_next, float *act_out, float *rew_out,
                                  uint8_t *term_out, int32_t *bad_index, void *stream)
{
    if (!idx || !ring_pos || !actions || !rewards || !terminated || !rows_s || !rows_next || !act_out || !rew_out || !term_out || !bad_index)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_offpolicy_stage_resolve: NULL argument");
    if (n < 1 || valid_rows < 1 || num_envs < 1 || slots < 1)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_offpolicy_stage_resolve: n, valid_rows, num_envs and slots must be >= 1");
    if (act_dim < 1 || act_dim > MAX_ACT) return rover_internal_fail(ROVER_ERR_INVALID, "rover_offpolicy_stage_resolve: act_dim must be in [1, 16]");
    if (!aligned_to(idx, 8) || !aligned_to(rows_s, 8) || !aligned_to(rows_next, 8))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_offpolicy_stage_resolve: idx, rows_s and rows_next must be 8-byte aligned");
    if (!aligned_to(ring_pos, 4) || !aligned_to(actions, 4) || !aligned_to(rewards, 4) || !aligned_to(act_out, 4) || !aligned_to(rew_out, 4) ||
        !aligned_to(bad_index, 4))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_offpolicy_stage_resolve: the 4-byte arrays must be 4-byte aligned");
    int dev;
    if (int rc = device_of(rows_s, &dev, true)) return rc;
    DeviceGuard guard(dev);
    ResolveArgs A;
    A.idx = idx; A.n = n; A.valid = valid_rows;
    A.num_envs = num_envs; A.slots = slots; A.act_dim = act_dim;
    A.pos = ring_pos; A.act = actions; A.rew = rewards; A.term = terminated;
    A.rows_s = rows_s; A.rows_n = rows_next; A.a = act_out; A.r = rew_out; A.t = term_out; A.bad = bad_index;
    hipLaunchKernelGGL(offpolicy_stage_resolve_kernel, dim3(cdiv(n, TT)), dim3(TT), 0, static_cast<hipStream_t>(stream), A);
    return launched("offpolicy_stage_resolve_kernel launch: %s");
}

int rover_offpolicy_stage_rows(const rover_scaler_hparams *h, const double *scaler, int32_t width, const float *x, int64_t x_rows,
                               const int64_t *src, int32_t n, float *out, int32_t *bad_index, void *stream)
{
    if (!h || !scaler || !x || !src || !out) return rover_internal_fail(ROVER_ERR_INVALID, "rover_offpolicy_stage_rows: NULL argument");
    if (width < 1 || width > MAX_W) return rover_internal_fail(ROVER_ERR_INVALID, "rover_offpolicy_stage_rows: width must be in [1, 1024]");
    if (n < 1 || x_rows < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_offpolicy_stage_rows: n and x_rows must be >= 1");
    if (!aligned_to(scaler, 8) || !aligned_to(src, 8))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_offpolicy_stage_rows: scaler and src must be 8-byte aligned");
    if (!aligned_to(x, 4) || !aligned_to(out, 4) || !aligned_to(bad_index, 4))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_offpolicy_stage_rows: x, out and bad_index must be 4-byte aligned");
    const uintptr_t px = reinterpret_cast<uintptr_t>(x), po = reinterpret_cast<uintptr_t>(out);
    const uintptr_t xb = sizeof(float) * (uintptr_t)x_rows * (uintptr_t)width, ob = sizeof(float) * (uintptr_t)n * (uintptr_t)width;
    if (px < po + ob && po < px + xb) return rover_internal_fail(ROVER_ERR_INVALID, "rover_offpolicy_stage_rows: out overlaps x");
    int dev;
    if (int rc = device_of(out, &dev, true)) return rc;
    DeviceGuard guard(dev);
    RowsArgs A;
    A.scaler = scaler; A.x = x; A.x_rows = x_rows; A.src = src; A.n = n; A.out = out; A.bad = bad_index; A.width = width;
    A.eps = h->eps; A.clip = h->clip;
    const int blocks = cdiv(n, WAVES);
    hipLaunchKernelGGL(offpolicy_stage_rows_kernel, dim3((unsigned)(blocks < ROWS_MAX_BLOCKS ? blocks : ROWS_MAX_BLOCKS)), dim3(TT), 0,
                       static_cast<hipStream_t>(stream), A);
    return launched("offpolicy_stage_rows_kernel launch: %s");
}

}  // extern "C"
