// td3_collect_kernels.hip -- the off-policy half of an env step in two launches (gfx950 / CDNA4, wave64): before env.step the actor
// on a ring slot of the replay memory, counter-based exploration noise and the clamp; after it the env's raw rows sanitised into the
// next ring slot, reward / terminated / ring_pos of the transition and the batch's row indices.  See include/rover_td3_collect.h
// for the contract.
//
// The network part is td3_actor_tile.hpp's (the single-network kernel of policy_kernels.hip restated, bit-identical to
// rover_policy_forward on the same rows).  One thing differs from that kernel: the epilogue.  The 16 x 16 lanes of waves 0 .. 3 that
// hold the final-layer sums go on to the draw, the noise and the clamp.  The record kernel and the host side of both entry points
// (checks, grid, launch) are offpolicy_collect.hpp's, shared with sac_collect_kernels.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_hip.h"
#include "../../include/rover_td3_collect.h"
#include "offpolicy_collect.hpp"
#include "rover_internal.hpp"
#include "td3_actor_tile.hpp"

namespace {

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

// the record kernel's launch struct (offpolicy_collect.hpp): no draws besides the indices
struct RecLaunch : RecFields {
    static constexpr bool DRAWS = false;
};

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
    if (int rc = collect_act_check("rover_td3_collect_act", actor, h, packed, obs, act_out, env_act_out, n, n_copies)) return rc;
    if (h->explore != 0 && h->explore != 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_act: explore must be 0 or 1");
    if (h->explore && !(h->action_low <= h->action_high))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_td3_collect_act: action_low > action_high");
    if (!is_reference_actor(actor, ROVER_ACT_NONE))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "rover_td3_collect_act: the actor must have the reference architecture with no "
                                                          "final activation");
    TdcLaunch L;
    L.hp = *h;
    L.mean_out = mean_out; L.act_out = act_out; L.env_act_out = env_act_out; L.eps_out = eps_out;
    return collect_act_launch("rover_td3_collect_act", rover_td3_collect_act_kernel, actor, L, packed, n_copies, counter, obs, n, stream);
}

int rover_td3_collect_record(const float *obs_raw, int32_t n, float *ring_slot_out, const float *rew, const uint8_t *terminated,
                             float *rew_out, uint8_t *term_out, int32_t *ring_pos_entry, int32_t ring_pos_value, int64_t *idx_out,
                             int32_t batch, int64_t mem_rows, const rover_td3_collect_hparams *h, uint64_t counter, void *stream)
{
    return collect_record<RecLaunch>("rover_td3_collect_record", obs_raw, n, ring_slot_out, rew, terminated, rew_out, term_out,
                                     ring_pos_entry, ring_pos_value, idx_out, batch, mem_rows, nullptr, h, counter, stream);
}

}  // extern "C"
