// td3_collect_kernels.hip -- the off-policy half of an env step in two launches (gfx950 / CDNA4, wave64): before env.step the actor
// on a ring slot of the replay memory, counter-based exploration noise and the clamp; after it the env's raw rows sanitised into the
// next ring slot, reward / terminated / ring_pos of the transition and the batch's row indices.  See include/rover_td3_collect.h
// for the contract.
//
// The network part is td3_actor_tile.hpp's (the single-network kernel of policy_kernels.hip restated, bit-identical to
// rover_policy_forward on the same rows).  One thing differs from that kernel: the epilogue.  The 16 x 16 lanes of waves 0 .. 3 that
// hold the final-layer sums go on to the draw, the noise and the clamp.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>


#include "../../include/rover_hip.h"
#include "../../include/rover_td3_collect.h"
#include "rover_internal.hpp"
#include "td3_actor_tile.hpp"

namespace {

constexpr uint32_t INDEX_TAG = 0x54335300u;   // "T3S\0": ... of the batch's row indices
constexpr int REC_THREADS = 256, REC_PER = 4; // record kernel: pieces (16 bytes, or one float on the scalar path) per thread

// torch.nan_to_num(x, nan = 0, posinf = FLT_MAX, neginf = 0): finite values (and -0) pass unchanged (rollout_kernels.hip)
__device__ __forceinline__ float sanitise(float x)
{
    if (x != x) return 0.0f;
    if (x == INFINITY) return FLT_MAX;
    if (x == -INFINITY) return 0.0f;
    return x;
}

struct TdcLaunch {
    int n_copies;              // replicas of the packed buffer; workgroup b reads replica b % n_copies
    unsigned copy_floats;
    rover_td3_collect_hparams hp;
    uint32_t ctr_lo, ctr_hi;
    float *mean_out, *act_out, *env_act_out, *eps_out;
};

__global__ __launch_bounds__(TDC_THREADS) void rover_td3_collect_act_kernel(rover_policy_desc d, TdcLaunch L,
                                                                            const float *__restrict__ packed,
                                                                            const float *__restrict__ obs, int n)
{
    extern __shared__ __align__(16) float lds[];
    Td3ActorLane p;
    if (!td3_actor_tile(d, packed, L.n_copies, L.copy_floats, obs, n, lds, p)) return;
    if (p.live && L.mean_out) L.mean_out[p.o] = p.y;

    // ---- exploration epilogue (td3.explore): noise_std * eps, * scale, + mean as three separate operations, then the clamp (a NaN
    // sum stays NaN, as under torch.clamp)
    float a = p.y;
    if (L.hp.explore) {
        const float eps = td3_noise_eps((uint32_t)L.hp.env_id_offset + (uint32_t)p.row, L.ctr_lo, L.ctr_hi, NOISE_TAG, p.c, L.hp.seed_lo,
                                        L.hp.seed_hi);
        a = td3_add_noise_clamp(p.y, L.hp.noise_std * eps, L.hp.noise_scale, L.hp.action_low, L.hp.action_high);
        if (p.live && L.eps_out) L.eps_out[p.o] = eps;
    }
    if (p.live) {
        L.act_out[p.o] = a;
        L.env_act_out[p.o] = a;
    }
}

struct RecLaunch {
    const float *rew;
    const uint8_t *terminated;
    float *rew_out;
    uint8_t *term_out;
    int32_t *ring_pos_entry;
    int32_t ring_pos_value;
    int64_t *idx_out;
    int batch;
    uint64_t mem_rows;
    uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi;
};

// VEC: both row pointers are 16-byte aligned.  Block b takes pieces [b * 1024, b * 1024 + 1024), thread t pieces t, t + 256, ...;
// the grid also covers n and batch threads for the record and the indices (blocks past the rows only do those).
template <bool VEC>
__global__ __launch_bounds__(REC_THREADS) void rover_td3_collect_record_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                                               size_t total, int n, RecLaunch R)
{
    const size_t gid = (size_t)blockIdx.x * REC_THREADS + threadIdx.x;
    const size_t base = (size_t)blockIdx.x * (REC_THREADS * REC_PER) + threadIdx.x;
    if (VEC) {
        const v4f *s4 = reinterpret_cast<const v4f *>(src);
        v4f *d4 = reinterpret_cast<v4f *>(dst);
        const size_t n4 = total >> 2;               // >= 241: a row is 965 floats
        if (base < n4) {
            v4f v[REC_PER];
#pragma unroll
            for (int u = 0; u < REC_PER; ++u) v[u] = __builtin_nontemporal_load(s4 + min(base + (size_t)u * REC_THREADS, n4 - 1));   // read once
#pragma unroll
            for (int u = 0; u < REC_PER; ++u) {
                const size_t i = base + (size_t)u * REC_THREADS;
                v4f s;
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j] = sanitise(v[u][j]);
                if (i < n4) d4[i] = s;              // a plain store: the next act launch reads this slot
            }
        }
        if (gid < (total & 3)) dst[4 * n4 + gid] = sanitise(src[4 * n4 + gid]);   // the floats behind the last whole piece
    } else {
#pragma unroll
        for (int u = 0; u < REC_PER; ++u) {
            const size_t i = base + (size_t)u * REC_THREADS;
            if (i < total) dst[i] = sanitise(src[i]);
        }
    }
    if (R.rew_out && gid < (size_t)n) {
        R.rew_out[gid] = R.rew[gid];
        R.term_out[gid] = R.terminated[gid] != 0 ? 1 : 0;
    }
    if (R.ring_pos_entry && gid == 0) *R.ring_pos_entry = R.ring_pos_value;
    if (R.idx_out && gid < (size_t)R.batch) {
        uint32_t w4[4];
        philox4x32((uint32_t)(gid >> 2), R.ctr_lo, R.ctr_hi, INDEX_TAG, R.seed_lo, R.seed_hi, w4);
        const uint32_t w = w4[gid & 3];
        R.idx_out[gid] = (int64_t)(((uint64_t)w * R.mem_rows) >> 32);   // mem_rows <= 2^32: the product fits 64 bits
    }
}

}  // namespace

extern "C" {

int rover_td3_collect_default_hparams(rover_td3_collect_hparams *h)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "hparams is NULL");
    memset(h, 0, sizeof(*h));
    h->seed_lo = 42u; h->seed_hi = 0u;
    h->env_id_offset = 0;
    h->explore = 0;
    h->noise_std = 0.0f; h->noise_scale = 1.0f;
    h->action_low = -1.0f; h->action_high = 1.0f;     // skrl TD3: the action space's bounds
    return ROVER_OK;
}

size_t rover_td3_collect_hparams_bytes(void) { return sizeof(rover_td3_collect_hparams); }

int rover_td3_collect_act(const rover_policy_desc *actor, const float *packed, int32_t n_copies, const rover_td3_collect_hparams *h,
                          uint64_t counter, const float *obs, int32_t n, float *mean_out, float *act_out, float *env_act_out,
                          float *eps_out, void *stream)
{
    if (!actor || !h) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_act: NULL descriptor / hparams");
    if (!packed || !obs || !act_out || !env_act_out) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_act: NULL required pointer");
    if (n < 1 || n_copies < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_act: n and n_copies must be >= 1");
    if (reinterpret_cast<uintptr_t>(packed) & 15) return rover_internal_fail(ROVER_ERR_INVALID, "packed weights must be 16-byte aligned");
    if (h->explore != 0 && h->explore != 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_act: explore must be 0 or 1");
    if (h->explore && !(h->action_low <= h->action_high))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_act: action_low > action_high");
    if (!is_reference_actor(actor))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "rover_td3_collect_act: the actor must have the reference architecture with no "
                                                          "final activation");
    TdcLaunch L;
    L.n_copies = n_copies;
    L.copy_floats = (unsigned)rover_policy_packed_floats(actor);
    L.hp = *h;
    L.ctr_lo = (uint32_t)(counter & 0xFFFFFFFFu);
    L.ctr_hi = (uint32_t)(counter >> 32);
    L.mean_out = mean_out; L.act_out = act_out; L.env_act_out = env_act_out; L.eps_out = eps_out;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(rover_td3_collect_act_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(rover_td3_collect_act_kernel, dim3(ceil_div(n, TDC_ROWS)), dim3(TDC_THREADS), LDS_BYTES,
                       static_cast<hipStream_t>(stream), *actor, L, packed, obs, n);
    e = hipGetLastError();
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "rover_td3_collect_act_kernel launch: %s", hipGetErrorString(e));
    return ROVER_OK;
}

int rover_td3_collect_record(const float *obs_raw, int32_t n, float *ring_slot_out, const float *rew, const uint8_t *terminated,
                             float *rew_out, uint8_t *term_out, int32_t *ring_pos_entry, int32_t ring_pos_value, int64_t *idx_out,
                             int32_t batch, int64_t mem_rows, const rover_td3_collect_hparams *h, uint64_t counter, void *stream)
{
    if (!obs_raw || !ring_slot_out) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: NULL rows");
    if (n < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: n must be >= 1");
    const size_t total = (size_t)n * OBS;
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(obs_raw), b = reinterpret_cast<uintptr_t>(ring_slot_out);
        if (a < b + total * sizeof(float) && b < a + total * sizeof(float))
            return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: ring_slot_out must not alias obs_raw");
    }
    const int given = (rew != nullptr) + (terminated != nullptr) + (rew_out != nullptr) + (term_out != nullptr);
    if (given != 0 && given != 4)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: rew, terminated, rew_out, term_out: all or none NULL");
    if (idx_out) {
        if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: hparams is NULL");
        if (batch < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: batch must be >= 1");
        if (mem_rows < 1 || mem_rows > ((int64_t)1 << 32))
            return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: mem_rows must lie in [1, 2^32]");
    }
    const bool vec = ((reinterpret_cast<uintptr_t>(obs_raw) | reinterpret_cast<uintptr_t>(ring_slot_out)) & 15) == 0;
    const size_t units = vec ? total >> 2 : total, per_block = (size_t)REC_THREADS * REC_PER;
    size_t blocks = (units + per_block - 1) / per_block;
    const size_t threads = (size_t)(idx_out && batch > n ? batch : n);
    if (blocks < (threads + REC_THREADS - 1) / REC_THREADS) blocks = (threads + REC_THREADS - 1) / REC_THREADS;
    if (blocks > 0x7FFFFFFFu) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_record: n too large");
    RecLaunch R;
    R.rew = rew; R.terminated = terminated; R.rew_out = rew_out; R.term_out = term_out;
    R.ring_pos_entry = ring_pos_entry; R.ring_pos_value = ring_pos_value;
    R.idx_out = idx_out; R.batch = idx_out ? batch : 0; R.mem_rows = idx_out ? (uint64_t)mem_rows : 1u;
    R.seed_lo = h ? h->seed_lo : 0u; R.seed_hi = h ? h->seed_hi : 0u;
    R.ctr_lo = (uint32_t)(counter & 0xFFFFFFFFu);
    R.ctr_hi = (uint32_t)(counter >> 32);
    if (vec)
        hipLaunchKernelGGL(rover_td3_collect_record_kernel<true>, dim3((unsigned)blocks), dim3(REC_THREADS), 0,
                           static_cast<hipStream_t>(stream), obs_raw, ring_slot_out, total, n, R);
    else
        hipLaunchKernelGGL(rover_td3_collect_record_kernel<false>, dim3((unsigned)blocks), dim3(REC_THREADS), 0,
                           static_cast<hipStream_t>(stream), obs_raw, ring_slot_out, total, n, R);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "rover_td3_collect_record_kernel launch: %s", hipGetErrorString(e));
    return ROVER_OK;
}

}  // extern "C"
