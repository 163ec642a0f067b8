// collect_record.hpp -- the transition record every collector's rows kernel carries, and the small host helpers that go with it
// (offpolicy_collect.hpp, dagger_collect_kernels.hip, dagger_conv_kernels.hip; dagger_kernels.hip through dagger_tail.hpp).
//
// It defines no tile or network constant and includes neither td3_actor_tile.hpp nor offpolicy_net.hpp, whose constants share
// names: a translation unit built on either of the two can include it.
#ifndef ROVER_COLLECT_RECORD_HPP
#define ROVER_COLLECT_RECORD_HPP

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/rover_hip.h"
#include "rover_internal.hpp"

namespace {

constexpr uint32_t INDEX_TAG = 0x54335300u;   // "T3S\0": word 3 of the Philox counter of the batch's row indices

// what a rows kernel does beside its rows: reward / terminated / ring_pos of the transition, the batch's row indices
struct RecFields {
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

// The device lines that act on the struct (reward, terminated, ring_pos; the Philox draw of a batch position) stay in each rows
// kernel's own text.  As device functions here they compile to other code: the compiler simplifies a callee on its own before it
// inlines it, which trades the kernels' ordered tests for unordered ones and adds two instructions to the index draw.

// a pixel that is NaN, +-inf or negative counts as `clip` (d >= 0 fails for NaN, -inf and every negative; +inf falls to the min)
__device__ __forceinline__ float depth_value(float d, float clip, float scale)
{
    const float v = d >= 0.0f ? d : clip;
    return scale * fminf(v, clip);
}

// rover_last_error() = "<fn><text><detail>": the three parts go through fixed formats, none of them is one
inline int collect_fail(int code, const char *fn, const char *text, const char *detail = "")
{
    char msg[384];
    snprintf(msg, sizeof(msg), "%s%s%s", fn, text, detail);
    return rover_internal_fail(code, "%s", msg);
}

inline bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}
inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// the DAgger rows entry points' refusals about the record
inline int rec_check(const char *fn, const float *rew, const uint8_t *terminated, const float *rew_out, const uint8_t *term_out,
                     const int64_t *idx_out, int32_t batch, int64_t mem_rows)
{
    const int given = (rew != nullptr) + (terminated != nullptr) + (rew_out != nullptr) + (term_out != nullptr);
    if (given != 0 && given != 4) return collect_fail(ROVER_ERR_INVALID, fn, ": rew, terminated, rew_out, term_out: all or none NULL");
    if (idx_out) {
        if (batch < 1) return collect_fail(ROVER_ERR_INVALID, fn, ": batch must be >= 1");
        if (mem_rows < 1 || mem_rows > ((int64_t)1 << 32)) return collect_fail(ROVER_ERR_INVALID, fn, ": mem_rows must lie in [1, 2^32]");
    }
    return ROVER_OK;
}

// `h` (a collector's hparams) gives the seed
template <class Hparams>
RecFields rec_fill(const Hparams *h, uint64_t counter, const float *rew, const uint8_t *terminated, float *rew_out, uint8_t *term_out,
                   int32_t *ring_pos_entry, int32_t ring_pos_value, int64_t *idx_out, int32_t batch, int64_t mem_rows)
{
    RecFields R = {};
    R.rew = rew; R.terminated = terminated; R.rew_out = rew_out; R.term_out = term_out;
    R.ring_pos_entry = ring_pos_entry; R.ring_pos_value = ring_pos_value;
    R.idx_out = idx_out; R.batch = idx_out ? batch : 0; R.mem_rows = idx_out ? (uint64_t)mem_rows : 1u;
    R.seed_lo = h->seed_lo; R.seed_hi = h->seed_hi;
    R.ctr_lo = (uint32_t)(counter & 0xFFFFFFFFu);
    R.ctr_hi = (uint32_t)(counter >> 32);
    return R;
}

}  // namespace

#endif  // ROVER_COLLECT_RECORD_HPP
