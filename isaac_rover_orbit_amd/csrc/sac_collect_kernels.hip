// sac_collect_kernels.hip -- the off-policy half of a SAC env step in two launches (gfx950 / CDNA4, wave64): before env.step the
// Gaussian actor on a ring slot of the replay memory, the counter-based draw, the clamp and the log-probability; after it the env's
// raw rows sanitised into the next ring slot, reward / terminated / ring_pos of the transition, the batch's row indices and the
// update's standard normal draws.  See include/rover_sac_collect.h for the contract.
//
//   rover_sac_collect_act_kernel     SAMPLE / MEAN: td3_actor_tile.hpp's forward (the device function rover_td3_collect_act runs), then
//                                    the Gaussian head of sac_kernels.hip on the 16 x 16 lanes of waves 0 .. 3 that hold the
//                                    final-layer sums.  The mode is a launch argument and the branch on it is wave-uniform.
//   rover_sac_collect_random_kernel  RANDOM: one lane per action value, no LDS, no actor
//   the record kernel                offpolicy_collect.hpp's, the one rover_td3_collect_record runs, with the four standard normals
//                                    per batch position turned on (SacRecLaunch::DRAWS)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_hip.h"
#include "../../include/rover_sac_collect.h"
#include "../../include/rover_td3_explore.h"
#include "offpolicy_collect.hpp"
#include "rover_internal.hpp"
#include "td3_actor_tile.hpp"
#include "train_math.hpp"

namespace {

constexpr int ACT_W = 2;                      // the SAC parameter vector fixes log_std at 2 floats (rover_sac.h)
constexpr float LS_MIN = -20.0f, LS_MAX = 2.0f, U_MIN = -1.0f, U_MAX = 1.0f;
constexpr float HALF_LN_2PI = 0.91893853320467274178f;

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
    const float u = unit_uniform((c & 2) ? ((c & 1) ? w4[3] : w4[2]) : ((c & 1) ? w4[1] : w4[0]));   // selects, not a private array
    const float t = 2.0f * u;
    const float a = -1.0f + t;
    R.act_out[e] = a;
    R.env_act_out[e] = a;
}

// the record kernel's launch struct (offpolicy_collect.hpp): the indices and four standard normals per batch position
struct SacRecLaunch {
    static constexpr bool DRAWS = true;
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
    if (int rc = collect_act_check("rover_sac_collect_act", actor, h, packed, obs, act_out, env_act_out, n, n_copies)) return rc;
    const int mode = h->mode;
    if (mode != ROVER_SAC_COLLECT_SAMPLE && mode != ROVER_SAC_COLLECT_MEAN && mode != ROVER_SAC_COLLECT_RANDOM)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_act: unknown mode");
    if (mode == ROVER_SAC_COLLECT_SAMPLE && !log_std) return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_act: SAMPLE needs log_std");
    if (!is_reference_actor(actor, ROVER_ACT_TANH) || actor->layers[5].N != ACT_W)
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "rover_sac_collect_act: the actor must have the reference architecture with two "
                                                          "tanh outputs");
    if (mode == ROVER_SAC_COLLECT_RANDOM) {
        SacRandomLaunch R;
        R.seed_lo = h->seed_lo; R.seed_hi = h->seed_hi;
        R.ctr_lo = (uint32_t)(counter & 0xFFFFFFFFu); R.ctr_hi = (uint32_t)(counter >> 32);
        R.id0 = (uint32_t)h->env_id_offset;
        R.act_out = act_out; R.env_act_out = env_act_out;
        if ((uint64_t)n * ACT_W > 0x7FFFFFFFu) return rover_internal_fail(ROVER_ERR_INVALID, "rover_sac_collect_act: n too large");
        const unsigned total = (unsigned)n * ACT_W;
        hipLaunchKernelGGL(rover_sac_collect_random_kernel, dim3((total + FLAT_THREADS - 1) / FLAT_THREADS), dim3(FLAT_THREADS), 0,
                           static_cast<hipStream_t>(stream), R, total);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "rover_sac_collect_random_kernel launch: %s", hipGetErrorString(e));
        return ROVER_OK;
    }
    SacActLaunch L;
    L.hp = *h;
    L.log_std = log_std;
    L.mean_out = mean_out; L.act_out = act_out; L.env_act_out = env_act_out;
    L.eps_out = eps_out; L.logp_out = logp_out; L.sigma_out = sigma_out;
    return collect_act_launch("rover_sac_collect_act", rover_sac_collect_act_kernel, actor, L, packed, n_copies, counter, obs, n, stream);
}

int rover_sac_collect_record(const float *obs_raw, int32_t n, float *ring_slot_out, const float *rew, const uint8_t *terminated,
                             float *rew_out, uint8_t *term_out, int32_t *ring_pos_entry, int32_t ring_pos_value, int64_t *idx_out,
                             int32_t batch, int64_t mem_rows, float *eps_out, const rover_sac_collect_hparams *h, uint64_t counter,
                             void *stream)
{
    return collect_record<SacRecLaunch>("rover_sac_collect_record", obs_raw, n, ring_slot_out, rew, terminated, rew_out, term_out,
                                        ring_pos_entry, ring_pos_value, idx_out, batch, mem_rows, eps_out, h, counter, stream);
}

}  // extern "C"
