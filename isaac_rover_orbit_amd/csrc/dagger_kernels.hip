// dagger_kernels.hip -- fused DAgger update of the depth student (gfx950 / CDNA4, wave64).
//
// One supervised step of the reference's policy network on student rows against the teacher's labels; see include/rover_dagger.h
// for the contract and the reduction order.  The network's forward, backward and weight gradients and the gather of the sampled
// rows are offpolicy_net.hpp's, shared with td3_kernels.hip and sac_kernels.hip, under this trainer's state type.  The imitation
// loss head, the gradient's norm, the final reduce into the device state, Adam, the argument checks and the workspace are
// dagger_tail.hpp's, shared with dagger_conv_kernels.hip; this file is the entry point that strings them together.  The
// collector's kernels are dagger_collect_kernels.hip's: offpolicy_net.hpp and td3_actor_tile.hpp give the same names to their
// constants, so one translation unit cannot include both.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_dagger.h"
#include "../../include/rover_hip.h"
#include "../../include/rover_policy.h"
#include "rover_internal.hpp"
#include "offpolicy_net.hpp"
#include "train_math.hpp"
#include "dagger_tail.hpp"

extern "C" {

int rover_dagger_default_hparams(rover_dagger_hparams *h)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "hparams is NULL");
    memset(h, 0, sizeof(*h));
    h->seed_lo = 42u; h->seed_hi = 0u;
    h->env_id_offset = 0;
    h->depth_clip = 10.0f; h->depth_scale = 0.1f;
    h->lr = 3e-4f;
    h->beta1 = 0.9f; h->beta2 = 0.999f; h->eps = 1e-8f;
    h->grad_norm_clip = 0.0f;
    return ROVER_OK;
}
size_t rover_dagger_hparams_bytes(void) { return sizeof(rover_dagger_hparams); }
size_t rover_dagger_state_bytes(void) { return sizeof(rover_dagger_state); }

size_t rover_dagger_param_floats(const rover_policy_desc *student)
{
    if (!is_net(student, false, ROVER_ACT_TANH, true)) return 0;
    return head_floats();
}
size_t rover_dagger_workspace_bytes(int32_t max_rows) { return max_rows > 0 ? sizeof(float) * ws_shared_floats(max_rows) : 0; }

int rover_dagger_update(const rover_policy_desc *student, const rover_dagger_hparams *h, float *params, float *grad, float *adam_m,
                        float *adam_v, const float *obs_ring, int32_t slots, int32_t num_envs, const int32_t *ring_pos,
                        const float *labels, const int64_t *idx, int32_t n, int64_t valid_rows, void *ws, size_t ws_bytes,
                        void *state, float *replicas, int32_t n_copies, float *dz_out, void *stream)
{
    if (int rc = update_check(student, h, params, grad, adam_m, adam_v, obs_ring, slots, num_envs, ring_pos, labels, idx, n, valid_rows,
                              ws, ws_bytes, rover_dagger_workspace_bytes(n), state, replicas, n_copies, nullptr))
        return rc;
    int dev;
    if (int rc = device_of(params, &dev)) return rc;
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    rover_dagger_state *st = static_cast<rover_dagger_state *>(state);
    Ws w = {};
    ws_carve(w, ws, n);
    const int P = (int)net_floats(false);
    const Net pi = net_at(student, params, false);
    if (int rc = gather(w, idx, n, valid_rows, num_envs, slots, ring_pos, nullptr, nullptr, nullptr, st, s)) return rc;
    FwdJob job = {pi, w.ro_s, nullptr, 0, &w.reg};
    if (int rc = forward<State>(&job, 1, obs_ring, n, s)) return rc;
    if (int rc = dagger_head(w, labels, idx, valid_rows, n, dz_out, s)) return rc;
    Region *regs[1] = {&w.reg};
    for (int l = NL - 1; l >= 1; --l)
        if (int rc = back_layer<State>(&pi, regs, 1, l, n, s)) return rc;
    if (int rc = wgrad<State>(&pi, regs, w.ro_s, 1, obs_ring, n, w.part, grad, s)) return rc;
    return dagger_tail(h, params, grad, adam_m, adam_v, P, P, w, n, st, replicas, n_copies, s);
}

}  // extern "C"
