// td3_explore_kernels.hip -- TD3's exploration switches and the smoothing draw (gfx950 / CDNA4, wave64).  See
// include/rover_td3_explore.h for the contract.
//
//   rover_td3_explore_act_kernel     OFF / GAUSSIAN / OU: td3_actor_tile.hpp's forward (the device function rover_td3_collect_act
//                                    runs), then the epilogue on the 16 x 16 lanes of waves 0 .. 3.  The mode is a launch argument
//                                    and the branches on it are wave-uniform.
//   rover_td3_explore_random_kernel  RANDOM: one lane per action value, no LDS, no actor
//   rover_td3_smooth_draw_kernel     one lane per (batch position, action pair)
// The act entry point's common checks and its launch are offpolicy_collect.hpp's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_hip.h"
#include "../../include/rover_td3_explore.h"
#include "offpolicy_collect.hpp"
#include "rover_internal.hpp"
#include "td3_actor_tile.hpp"

namespace {

struct TdxLaunch {
    int n_copies;              // replicas of the packed buffer; workgroup b reads replica b % n_copies
    unsigned copy_floats;
    rover_td3_explore_hparams hp;
    uint32_t ctr_lo, ctr_hi;
    float *ou_state, *mean_out, *act_out, *env_act_out, *eps_out;
};

__global__ __launch_bounds__(TDC_THREADS) void rover_td3_explore_act_kernel(rover_policy_desc d, TdxLaunch L,
                                                                            const float *__restrict__ packed,
                                                                            const float *__restrict__ obs, int n)
{
    extern __shared__ __align__(16) float lds[];
    Td3ActorLane p;
    if (!td3_actor_tile(d, packed, L.n_copies, L.copy_floats, obs, n, lds, p)) return;
    if (p.live && L.mean_out) L.mean_out[p.o] = p.y;

    float a = p.y;
    if (L.hp.mode != ROVER_TD3_EXPLORE_OFF) {
        const bool ou = L.hp.mode == ROVER_TD3_EXPLORE_OU;
        const float x = ou && p.live ? L.ou_state[p.o] : 0.0f;   // requested in front of the draw, which hides it
        const float eps = td3_noise_eps((uint32_t)L.hp.env_id_offset + (uint32_t)p.row, L.ctr_lo, L.ctr_hi, NOISE_TAG, p.c, L.hp.seed_lo,
                                        L.hp.seed_hi);
        float noise;
        if (ou) {   // skrl's OrnsteinUhlenbeckNoise.sample: five separate fp32 operations (the build has no FMA contraction)
            const float t = x * L.hp.ou_theta;
            const float x1 = x - t;
            const float s = L.hp.ou_sigma * eps;
            const float xn = x1 + s;
            noise = L.hp.ou_base_scale * xn;
            if (p.live) L.ou_state[p.o] = xn;
        } else {
            noise = L.hp.noise_std * eps;
        }
        a = td3_add_noise_clamp(p.y, noise, L.hp.noise_scale, L.hp.action_low, L.hp.action_high);
        if (p.live && L.eps_out) L.eps_out[p.o] = eps;
    }
    if (p.live) {
        L.act_out[p.o] = a;
        L.env_act_out[p.o] = a;
    }
}

struct RandomLaunch {
    uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi, id0;
    float low, range;          // range = high - low, rounded once on the host
    float *act_out, *env_act_out;
};

// lane -> (row, column), the column fastest; the lanes of one quad of columns repeat that quad's Philox block, which is cheaper
// than passing its words between lanes at these sizes
__global__ __launch_bounds__(FLAT_THREADS) void rover_td3_explore_random_kernel(RandomLaunch R, unsigned total, unsigned A)
{
    const unsigned e = blockIdx.x * FLAT_THREADS + threadIdx.x;
    if (e >= total) return;
    const unsigned row = e / A, c = e - row * A;
    uint32_t w4[4];
    philox4x32(R.id0 + row, R.ctr_lo, R.ctr_hi, ROVER_TD3_TAG_RANDOM | (c >> 2), R.seed_lo, R.seed_hi, w4);
    const float u = unit_uniform((c & 2) ? ((c & 1) ? w4[3] : w4[2]) : ((c & 1) ? w4[1] : w4[0]));   // selects, not a private array
    const float t = R.range * u;
    const float a = R.low + t;
    R.act_out[e] = a;
    R.env_act_out[e] = a;
}

__global__ __launch_bounds__(FLAT_THREADS) void rover_td3_smooth_draw_kernel(uint32_t seed_lo, uint32_t seed_hi, uint32_t ctr_lo,
                                                                             uint32_t ctr_hi, float std, float *__restrict__ out,
                                                                             unsigned pairs_total, unsigned pairs)
{
    const unsigned e = blockIdx.x * FLAT_THREADS + threadIdx.x;
    if (e >= pairs_total) return;
    const unsigned i = e / pairs, p = e - i * pairs;
    uint32_t w4[4];
    philox4x32(i, ctr_lo, ctr_hi, ROVER_TD3_TAG_SMOOTH | p, seed_lo, seed_hi, w4);
    float e0, e1;
    // normal_pair's two lines (offpolicy_collect.hpp) written out, not called: through one more inlined function the compiler
    // commutes the operands of six v_xor of the Philox rounds, and this kernel's instruction stream is kept as it was
    box_muller(w4[0], w4[1], e0, e1);
    out[2 * (size_t)e] = std * e0;
    out[2 * (size_t)e + 1] = std * e1;
}

}  // namespace

extern "C" {

int rover_td3_explore_default_hparams(rover_td3_explore_hparams *h)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "hparams is NULL");
    memset(h, 0, sizeof(*h));
    h->seed_lo = 42u; h->seed_hi = 0u;
    h->env_id_offset = 0;
    h->mode = ROVER_TD3_EXPLORE_OFF;
    h->noise_std = 0.0f; h->noise_scale = 1.0f;
    h->ou_theta = 0.15f; h->ou_sigma = 0.2f; h->ou_base_scale = 1.0f;   // skrl OrnsteinUhlenbeckNoise
    h->action_low = -1.0f; h->action_high = 1.0f;
    return ROVER_OK;
}

size_t rover_td3_explore_hparams_bytes(void) { return sizeof(rover_td3_explore_hparams); }

int rover_td3_explore_act(const rover_policy_desc *actor, const float *packed, int32_t n_copies, const rover_td3_explore_hparams *h,
                          uint64_t counter, const float *obs, int32_t n, float *ou_state, float *mean_out, float *act_out,
                          float *env_act_out, float *eps_out, void *stream)
{
    if (int rc = collect_act_check("rover_td3_explore_act", actor, h, packed, obs, act_out, env_act_out, n, n_copies)) return rc;
    const int mode = h->mode;
    if (mode != ROVER_TD3_EXPLORE_OFF && mode != ROVER_TD3_EXPLORE_GAUSSIAN && mode != ROVER_TD3_EXPLORE_OU && mode != ROVER_TD3_EXPLORE_RANDOM)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_explore_act: unknown mode");
    if (mode != ROVER_TD3_EXPLORE_OFF && !(h->action_low <= h->action_high))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_explore_act: action_low > action_high");
    if (mode == ROVER_TD3_EXPLORE_OU && !ou_state) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_explore_act: OU needs ou_state");
    if (!is_reference_actor(actor, ROVER_ACT_NONE))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "rover_td3_explore_act: the actor must have the reference architecture with no "
                                                          "final activation");
    if (mode == ROVER_TD3_EXPLORE_RANDOM) {
        RandomLaunch R;
        R.seed_lo = h->seed_lo; R.seed_hi = h->seed_hi;
        R.ctr_lo = (uint32_t)(counter & 0xFFFFFFFFu); R.ctr_hi = (uint32_t)(counter >> 32);
        R.id0 = (uint32_t)h->env_id_offset;
        R.low = h->action_low; R.range = h->action_high - h->action_low;
        R.act_out = act_out; R.env_act_out = env_act_out;
        const unsigned A = (unsigned)actor->layers[5].N;
        if ((uint64_t)n * A > 0x7FFFFFFFu) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_explore_act: n too large");
        const unsigned total = (unsigned)n * A;
        hipLaunchKernelGGL(rover_td3_explore_random_kernel, dim3((total + FLAT_THREADS - 1) / FLAT_THREADS), dim3(FLAT_THREADS), 0,
                           static_cast<hipStream_t>(stream), R, total, A);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "rover_td3_explore_random_kernel launch: %s", hipGetErrorString(e));
        return ROVER_OK;
    }
    TdxLaunch L;
    L.hp = *h;
    L.ou_state = mode == ROVER_TD3_EXPLORE_OU ? ou_state : nullptr;
    L.mean_out = mean_out; L.act_out = act_out; L.env_act_out = env_act_out; L.eps_out = eps_out;
    return collect_act_launch("rover_td3_explore_act", rover_td3_explore_act_kernel, actor, L, packed, n_copies, counter, obs, n, stream);
}

int rover_td3_smooth_draw(uint32_t seed_lo, uint32_t seed_hi, uint64_t counter, float std, float *noise_out, int32_t n, int32_t A,
                          void *stream)
{
    if (!noise_out) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_smooth_draw: noise_out is NULL");
    if (n < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_smooth_draw: n must be >= 1");
    if (A < 2 || A > 16 || (A & 1)) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_smooth_draw: A must be even and lie in [2, 16]");
    if (!(std >= 0.0f)) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_smooth_draw: std must be >= 0");
    const unsigned pairs = (unsigned)A / 2;
    if ((uint64_t)n * pairs > 0x7FFFFFFFu) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_smooth_draw: n too large");
    const unsigned total = (unsigned)n * pairs;
    hipLaunchKernelGGL(rover_td3_smooth_draw_kernel, dim3((total + FLAT_THREADS - 1) / FLAT_THREADS), dim3(FLAT_THREADS), 0,
                       static_cast<hipStream_t>(stream), seed_lo, seed_hi, (uint32_t)(counter & 0xFFFFFFFFu), (uint32_t)(counter >> 32), std,
                       noise_out, total, pairs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "rover_td3_smooth_draw_kernel launch: %s", hipGetErrorString(e));
    return ROVER_OK;
}

}  // extern "C"
