// sac_collect_kernels.hip -- the off-policy half of a SAC env step in two launches (gfx950 / CDNA4, wave64): before env.step the
// Gaussian actor on a ring slot of the replay memory, the counter-based draw, the clamp and the log-probability; after it the env's
// raw rows sanitised into the next ring slot, reward / terminated / ring_pos of the transition, the batch's row indices and the
// update's standard normal draws.  See include/rover_sac_collect.h for the contract.
//
//   rover_sac_collect_act_kernel     SAMPLE / MEAN: td3_actor_tile.hpp's forward (the device function rover_td3_collect_act runs), then
//                                    the Gaussian head of sac_kernels.hip on the 16 x 16 lanes of waves 0 .. 3 that hold the
//                                    final-layer sums.  The mode is a launch argument and the branch on it is wave-uniform.
//   rover_sac_collect_random_kernel  RANDOM: one lane per action value, no LDS, no actor
//   rover_sac_collect_record_kernel  rover_td3_collect_record_kernel restated (td3_collect_kernels.hip stays byte for byte what it
//                                    was), plus four standard normals per batch position
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_hip.h"
#include "../../include/rover_sac_collect.h"
#include "../../include/rover_td3_explore.h"
#include "rover_internal.hpp"
#include "td3_actor_tile.hpp"
#include "train_math.hpp"

namespace {

constexpr int ACT_W = 2;                      // the SAC parameter vector fixes log_std at 2 floats (rover_sac.h)
constexpr uint32_t INDEX_TAG = 0x54335300u;   // "T3S\0": word 3 of the Philox counter of the batch's row indices (td3_collect_kernels.hip)
constexpr int FLAT_THREADS = 256;             // the random kernel
constexpr int REC_THREADS = 256, REC_PER = 4; // record kernel: pieces (16 bytes, or one float on the scalar path) per thread
constexpr float LS_MIN = -20.0f, LS_MAX = 2.0f, U_MIN = -1.0f, U_MAX = 1.0f;
constexpr float HALF_LN_2PI = 0.91893853320467274178f;

// torch.nan_to_num(x, nan = 0, posinf = FLT_MAX, neginf = 0): finite values (and -0) pass unchanged (rollout_kernels.hip)
__device__ __forceinline__ float sanitise(float x)
{
    if (x != x) return 0.0f;
    if (x == INFINITY) return FLT_MAX;
    if (x == -INFINITY) return 0.0f;
    return x;
}

struct SacActLaunch {
    int n_copies;              // replicas of the packed buffer; workgroup b reads replica b % n_copies
    unsigned copy_floats;
    rover_sac_collect_hparams hp;
    uint32_t ctr_lo, ctr_hi;
    const float *log_std;
    float *mean_out, *act_out, *env_act_out, *eps_out, *logp_out, *sigma_out;
};

__global__ __launch_bounds__(TDC_THREADS) void rover_sac_collect_act_kernel(rover_policy_desc d, SacActLaunch L,
                                                                            const float *__restrict__ packed,
                                                                            const float *__restrict__ obs, int n)
{
    extern __shared__ __align__(16) float lds[];
    Td3ActorLane p;
    if (!td3_actor_tile(d, packed, L.n_copies, L.copy_floats, obs, n, lds, p)) return;
    const float mu = rv_tanhf(p.y);
    if (p.live && L.mean_out) L.mean_out[p.o] = mu;

    // ---- the Gaussian head (sac_gauss_head_kernel's order): every line one fp32 operation, the build contracts nothing
    float a = mu;
    if (L.hp.mode == ROVER_SAC_COLLECT_SAMPLE) {
        const float ls = tclamp(L.log_std[p.c & (ACT_W - 1)], LS_MIN, LS_MAX);   // lanes of columns >= 2 are not live: any valid address
        const float sigma = rv_expf(ls);
        const float eps = td3_noise_eps((uint32_t)L.hp.env_id_offset + (uint32_t)p.row, L.ctr_lo, L.ctr_hi, ROVER_SAC_TAG_ACTION, p.c,
                                        L.hp.seed_lo, L.hp.seed_hi);
        const float s = sigma * eps;
        const float x = mu + s;
        const float u = tclamp(x, U_MIN, U_MAX);
        const float t = (u - mu) / sigma;
        const float tt = t * t;
        const float h = -0.5f * tt;
        const float term = (h - ls) - HALF_LN_2PI;
        // lane (r, c) is lane 16 r + c of its wave: column 1's term and sigma sit one lane up from column 0's
        const float term1 = __shfl_down(term, 1);
        const float sigma1 = __shfl_down(sigma, 1);
        a = u;
        if (p.live && L.eps_out) L.eps_out[p.o] = eps;
        if (p.live && p.c == 0 && L.logp_out) L.logp_out[p.row] = term + term1;      // column 0 first
        if (L.sigma_out && blockIdx.x == 0 && threadIdx.x == 0) {
            L.sigma_out[0] = sigma;
            L.sigma_out[1] = sigma1;
        }
    }
    if (p.live) {
        L.act_out[p.o] = a;
        L.env_act_out[p.o] = a;
    }
}

struct SacRandomLaunch {
    uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi, id0;
    float *act_out, *env_act_out;
};

// lane -> (row, column), the column fastest; the two lanes of a row repeat the row's Philox block (rover_td3_explore_random_kernel)
__global__ __launch_bounds__(FLAT_THREADS) void rover_sac_collect_random_kernel(SacRandomLaunch R, unsigned total)
{
    const unsigned e = blockIdx.x * FLAT_THREADS + threadIdx.x;
    if (e >= total) return;
    const unsigned row = e / ACT_W, c = e - row * ACT_W;
    uint32_t w4[4];
    philox4x32(R.id0 + row, R.ctr_lo, R.ctr_hi, ROVER_SAC_TAG_RANDOM | (c >> 2), R.seed_lo, R.seed_hi, w4);
    const uint32_t w = (c & 2) ? ((c & 1) ? w4[3] : w4[2]) : ((c & 1) ? w4[1] : w4[0]);   // selects, not a private array
    const float u = ((float)(w >> 9) + 0.5f) * 0x1p-23f;   // exact, inside (0, 1)
    const float t = 2.0f * u;
    const float a = -1.0f + t;
    R.act_out[e] = a;
    R.env_act_out[e] = a;
}

struct SacRecLaunch {
    const float *rew;
    const uint8_t *terminated;
    float *rew_out;
    uint8_t *term_out;
    int32_t *ring_pos_entry;
    int32_t ring_pos_value;
    int64_t *idx_out;
    float *eps_out;
    int batch;
    uint64_t mem_rows;
    uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi;
};

// the standard normal pair of one Philox block: rover_td3_smooth_draw_kernel's text at std = 1
__device__ __forceinline__ void normal_pair(uint32_t i, uint32_t ctr_lo, uint32_t ctr_hi, uint32_t tag, uint32_t seed_lo, uint32_t seed_hi,
                                            float &e0, float &e1)
{
    uint32_t w4[4];
    philox4x32(i, ctr_lo, ctr_hi, tag, seed_lo, seed_hi, w4);
    const float u1 = ((float)(w4[0] >> 9) + 0.5f) * 0x1p-23f, u2 = ((float)(w4[1] >> 9) + 0.5f) * 0x1p-23f;   // exact, inside (0, 1)
    const float rho = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    e0 = rho * cs;
    e1 = rho * sn;
}

// VEC: both row pointers are 16-byte aligned.  Block b takes pieces [b * 1024, b * 1024 + 1024), thread t pieces t, t + 256, ...;
// the grid also covers n and batch threads for the record, the indices and the draws (blocks past the rows only do those).
template <bool VEC>
__global__ __launch_bounds__(REC_THREADS) void rover_sac_collect_record_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                                               size_t total, int n, SacRecLaunch R)
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
    if (gid < (size_t)R.batch) {
        if (R.idx_out) {
            uint32_t w4[4];
            philox4x32((uint32_t)(gid >> 2), R.ctr_lo, R.ctr_hi, INDEX_TAG, R.seed_lo, R.seed_hi, w4);
            const uint32_t w = w4[gid & 3];
            R.idx_out[gid] = (int64_t)(((uint64_t)w * R.mem_rows) >> 32);   // mem_rows <= 2^32: the product fits 64 bits
        }
        if (R.eps_out) {
            float e0, e1, e2, e3;
            normal_pair((uint32_t)gid, R.ctr_lo, R.ctr_hi, ROVER_TD3_TAG_SMOOTH | 0u, R.seed_lo, R.seed_hi, e0, e1);
            normal_pair((uint32_t)gid, R.ctr_lo, R.ctr_hi, ROVER_TD3_TAG_SMOOTH | 1u, R.seed_lo, R.seed_hi, e2, e3);
            reinterpret_cast<v4f *>(R.eps_out)[gid] = (v4f){e0, e1, e2, e3};   // one 16-byte store (eps_out is 16-byte aligned)
        }
    }
}

// the shapes the act kernel is written for (rover_policy_default_desc(2, tanh)): td3_actor_tile.hpp's check with the tanh head
bool is_reference_sac_actor(const rover_policy_desc *d)
{
    if (d->obs_dim != OBS || d->prop_dim != PROP || d->enc_offset != ENC_OFF || d->enc_dim != 961 || d->n_enc != 2 || d->n_mlp != 4) return false;
    const int K[6] = {961, 80, 64, 256, 160, 128}, N[5] = {80, 60, 256, 160, 128};
    for (int i = 0; i < 6; ++i) {
        if (d->layers[i].K != K[i]) return false;
        if (i < 5 && (d->layers[i].N != N[i] || d->layers[i].act != ROVER_ACT_LEAKY_RELU)) return false;
        if ((d->layers[i].split_k != 0) != (i == 0 || i == 5)) return false;
    }
    return d->layers[5].N == ACT_W && d->layers[5].act == ROVER_ACT_TANH;
}

}  // namespace

extern "C" {

int rover_sac_collect_default_hparams(rover_sac_collect_hparams *h)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "hparams is NULL");
    memset(h, 0, sizeof(*h));
    h->seed_lo = 42u; h->seed_hi = 0u;
    h->env_id_offset = 0;
    h->mode = ROVER_SAC_COLLECT_SAMPLE;
    return ROVER_OK;
}

size_t rover_sac_collect_hparams_bytes(void) { return sizeof(rover_sac_collect_hparams); }

int rover_sac_collect_act(const rover_policy_desc *actor, const float *packed, int32_t n_copies, const float *log_std,
                          const rover_sac_collect_hparams *h, uint64_t counter, const float *obs, int32_t n, float *mean_out,
                          float *act_out, float *env_act_out, float *eps_out, float *logp_out, float *sigma_out, void *stream)
{
    if (!actor || !h) return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_act: NULL descriptor / hparams");
    if (!packed || !obs || !act_out || !env_act_out) return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_act: NULL required pointer");
    if (n < 1 || n_copies < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_act: n and n_copies must be >= 1");
    if (reinterpret_cast<uintptr_t>(packed) & 15) return rover_internal_fail(ROVER_ERR_INVALID, "packed weights must be 16-byte aligned");
    const int mode = h->mode;
    if (mode != ROVER_SAC_COLLECT_SAMPLE && mode != ROVER_SAC_COLLECT_MEAN && mode != ROVER_SAC_COLLECT_RANDOM)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_act: unknown mode");
    if (mode == ROVER_SAC_COLLECT_SAMPLE && !log_std) return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_act: SAMPLE needs log_std");
    if (!is_reference_sac_actor(actor))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "rover_sac_collect_act: the actor must have the reference architecture with two "
                                                          "tanh outputs");
    const uint32_t ctr_lo = (uint32_t)(counter & 0xFFFFFFFFu), ctr_hi = (uint32_t)(counter >> 32);
    hipError_t e;
    if (mode == ROVER_SAC_COLLECT_RANDOM) {
        SacRandomLaunch R;
        R.seed_lo = h->seed_lo; R.seed_hi = h->seed_hi; R.ctr_lo = ctr_lo; R.ctr_hi = ctr_hi;
        R.id0 = (uint32_t)h->env_id_offset;
        R.act_out = act_out; R.env_act_out = env_act_out;
        if ((uint64_t)n * ACT_W > 0x7FFFFFFFu) return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_act: n too large");
        const unsigned total = (unsigned)n * ACT_W;
        hipLaunchKernelGGL(rover_sac_collect_random_kernel, dim3((total + FLAT_THREADS - 1) / FLAT_THREADS), dim3(FLAT_THREADS), 0,
                           static_cast<hipStream_t>(stream), R, total);
        e = hipGetLastError();
        if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "rover_sac_collect_random_kernel launch: %s", hipGetErrorString(e));
        return ROVER_OK;
    }
    SacActLaunch L;
    L.n_copies = n_copies;
    L.copy_floats = (unsigned)rover_policy_packed_floats(actor);
    L.hp = *h;
    L.ctr_lo = ctr_lo; L.ctr_hi = ctr_hi;
    L.log_std = log_std;
    L.mean_out = mean_out; L.act_out = act_out; L.env_act_out = env_act_out;
    L.eps_out = eps_out; L.logp_out = logp_out; L.sigma_out = sigma_out;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(rover_sac_collect_act_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)LDS_BYTES);
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(rover_sac_collect_act_kernel, dim3(ceil_div(n, TDC_ROWS)), dim3(TDC_THREADS), LDS_BYTES,
                       static_cast<hipStream_t>(stream), *actor, L, packed, obs, n);
    e = hipGetLastError();
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "rover_sac_collect_act_kernel launch: %s", hipGetErrorString(e));
    return ROVER_OK;
}

int rover_sac_collect_record(const float *obs_raw, int32_t n, float *ring_slot_out, const float *rew, const uint8_t *terminated,
                             float *rew_out, uint8_t *term_out, int32_t *ring_pos_entry, int32_t ring_pos_value, int64_t *idx_out,
                             int32_t batch, int64_t mem_rows, float *eps_out, const rover_sac_collect_hparams *h, uint64_t counter,
                             void *stream)
{
    if (!obs_raw || !ring_slot_out) return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_record: NULL rows");
    if (n < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_record: n must be >= 1");
    const size_t total = (size_t)n * OBS;
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(obs_raw), b = reinterpret_cast<uintptr_t>(ring_slot_out);
        if (a < b + total * sizeof(float) && b < a + total * sizeof(float))
            return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_record: ring_slot_out must not alias obs_raw");
    }
    const int given = (rew != nullptr) + (terminated != nullptr) + (rew_out != nullptr) + (term_out != nullptr);
    if (given != 0 && given != 4)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_record: rew, terminated, rew_out, term_out: all or none NULL");
    const bool draws = idx_out || eps_out;
    if (draws) {
        if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_record: hparams is NULL");
        if (batch < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_record: batch must be >= 1");
    }
    if (idx_out && (mem_rows < 1 || mem_rows > ((int64_t)1 << 32)))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_record: mem_rows must lie in [1, 2^32]");
    if (reinterpret_cast<uintptr_t>(eps_out) & 15)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_record: eps_out must be 16-byte aligned");
    const bool vec = ((reinterpret_cast<uintptr_t>(obs_raw) | reinterpret_cast<uintptr_t>(ring_slot_out)) & 15) == 0;
    const size_t units = vec ? total >> 2 : total, per_block = (size_t)REC_THREADS * REC_PER;
    size_t blocks = (units + per_block - 1) / per_block;
    const size_t threads = (size_t)(draws && batch > n ? batch : n);
    if (blocks < (threads + REC_THREADS - 1) / REC_THREADS) blocks = (threads + REC_THREADS - 1) / REC_THREADS;
    if (blocks > 0x7FFFFFFFu) return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_record: n too large");
    SacRecLaunch R;
    R.rew = rew; R.terminated = terminated; R.rew_out = rew_out; R.term_out = term_out;
    R.ring_pos_entry = ring_pos_entry; R.ring_pos_value = ring_pos_value;
    R.idx_out = idx_out; R.eps_out = eps_out; R.batch = draws ? batch : 0; R.mem_rows = idx_out ? (uint64_t)mem_rows : 1u;
    R.seed_lo = h ? h->seed_lo : 0u; R.seed_hi = h ? h->seed_hi : 0u;
    R.ctr_lo = (uint32_t)(counter & 0xFFFFFFFFu);
    R.ctr_hi = (uint32_t)(counter >> 32);
    if (vec)
        hipLaunchKernelGGL(rover_sac_collect_record_kernel<true>, dim3((unsigned)blocks), dim3(REC_THREADS), 0,
                           static_cast<hipStream_t>(stream), obs_raw, ring_slot_out, total, n, R);
    else
        hipLaunchKernelGGL(rover_sac_collect_record_kernel<false>, dim3((unsigned)blocks), dim3(REC_THREADS), 0,
                           static_cast<hipStream_t>(stream), obs_raw, ring_slot_out, total, n, R);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "rover_sac_collect_record_kernel launch: %s", hipGetErrorString(e));
    return ROVER_OK;
}

}  // extern "C"
