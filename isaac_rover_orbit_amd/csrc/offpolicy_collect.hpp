// offpolicy_collect.hpp -- what the off-policy transition collectors share (td3_collect_kernels.hip, td3_explore_kernels.hip,
// sac_collect_kernels.hip): the record kernel, the batch's index stream, the standard normal pair of one Philox block, and the host
// side of the act and record entry points (argument checks, grid sizing, launch).  The index stream's tag, the record's
// members (RecFields) and collect_fail are collect_record.hpp's, which the DAgger collectors include too.
//
//   offpolicy_collect_record_kernel  the env's raw rows sanitised into a ring slot, reward / terminated / ring_pos of the transition,
//                                    the batch's row indices and, for a launch struct with DRAWS, four standard normals per batch
//                                    position.  A template on the trainer's launch struct (RecLaunch, SacRecLaunch), so the two
//                                    trainers' kernels keep different names in a trace and in the library.
//
// The collectors include this one text; what differs between them (the act kernels' epilogues, the random kernels, the launch
// structs, the hparams and the entry points) stays in their files.  The host helpers take the entry point's name, so every message of
// rover_last_error() reads as it did when each entry point had its own copy.
#ifndef ROVER_OFFPOLICY_COLLECT_HPP
#define ROVER_OFFPOLICY_COLLECT_HPP

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/rover_hip.h"
#include "../../include/rover_td3_explore.h"
#include "collect_record.hpp"
#include "rover_internal.hpp"
#include "td3_actor_tile.hpp"

namespace {

constexpr int REC_THREADS = 256, REC_PER = 4; // record kernel: pieces (16 bytes, or one float on the scalar path) per thread
constexpr int FLAT_THREADS = 256;             // the random and draw kernels: one lane per value or pair

// the standard normal pair of one Philox block
__device__ __forceinline__ void normal_pair(uint32_t i, uint32_t ctr_lo, uint32_t ctr_hi, uint32_t tag, uint32_t seed_lo, uint32_t seed_hi,
                                            float &e0, float &e1)
{
    uint32_t w4[4];
    philox4x32(i, ctr_lo, ctr_hi, tag, seed_lo, seed_hi, w4);
    box_muller(w4[0], w4[1], e0, e1);
}

// VEC: both row pointers are 16-byte aligned.  Block b takes pieces [b * 1024, b * 1024 + 1024), thread t pieces t, t + 256, ...;
// the grid also covers n and batch threads for the record, the indices and the draws (blocks past the rows only do those).
template <bool VEC, class Launch>
__global__ __launch_bounds__(REC_THREADS) void offpolicy_collect_record_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                                               size_t total, int n, Launch R)
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
    // without DRAWS the index is the only draw and its pointer is tested first, in front of the batch test: each trainer's kernel
    // keeps the order of scalar tests, and with it the instruction stream, it had as its own text (profiles/collect_share_isa.txt)
    if ((Launch::DRAWS || R.idx_out) && gid < (size_t)R.batch) {
        if (!Launch::DRAWS || R.idx_out) {
            uint32_t w4[4];
            philox4x32((uint32_t)(gid >> 2), R.ctr_lo, R.ctr_hi, INDEX_TAG, R.seed_lo, R.seed_hi, w4);
            const uint32_t w = w4[gid & 3];
            R.idx_out[gid] = (int64_t)(((uint64_t)w * R.mem_rows) >> 32);   // mem_rows <= 2^32: the product fits 64 bits
        }
        if constexpr (Launch::DRAWS) {
            if (R.eps_out) {
                float e0, e1, e2, e3;
                normal_pair((uint32_t)gid, R.ctr_lo, R.ctr_hi, ROVER_TD3_TAG_SMOOTH | 0u, R.seed_lo, R.seed_hi, e0, e1);
                normal_pair((uint32_t)gid, R.ctr_lo, R.ctr_hi, ROVER_TD3_TAG_SMOOTH | 1u, R.seed_lo, R.seed_hi, e2, e3);
                reinterpret_cast<v4f *>(R.eps_out)[gid] = (v4f){e0, e1, e2, e3};   // one 16-byte store (eps_out is 16-byte aligned)
            }
        }
    }
}

// The record entry points: argument checks, the vector / scalar choice, the grid, the launch struct and the launch.  `eps_out` is
// NULL for a Launch without DRAWS; `h` (any collector's hparams) gives the seed.
template <class Launch, class Hparams>
int collect_record(const char *fn, const float *obs_raw, int32_t n, float *ring_slot_out, const float *rew, const uint8_t *terminated,
                   float *rew_out, uint8_t *term_out, int32_t *ring_pos_entry, int32_t ring_pos_value, int64_t *idx_out, int32_t batch,
                   int64_t mem_rows, float *eps_out, const Hparams *h, uint64_t counter, void *stream)
{
    if (!obs_raw || !ring_slot_out) return collect_fail(ROVER_ERR_INVALID, fn, ": NULL rows");
    if (n < 1) return collect_fail(ROVER_ERR_INVALID, fn, ": n must be >= 1");
    const size_t total = (size_t)n * OBS;
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(obs_raw), b = reinterpret_cast<uintptr_t>(ring_slot_out);
        if (a < b + total * sizeof(float) && b < a + total * sizeof(float))
            return collect_fail(ROVER_ERR_INVALID, fn, ": ring_slot_out must not alias obs_raw");
    }
    const int given = (rew != nullptr) + (terminated != nullptr) + (rew_out != nullptr) + (term_out != nullptr);
    if (given != 0 && given != 4) return collect_fail(ROVER_ERR_INVALID, fn, ": rew, terminated, rew_out, term_out: all or none NULL");
    const bool draws = idx_out || eps_out;
    if (draws) {
        if (!h) return collect_fail(ROVER_ERR_INVALID, fn, ": hparams is NULL");
        if (batch < 1) return collect_fail(ROVER_ERR_INVALID, fn, ": batch must be >= 1");
    }
    if (idx_out && (mem_rows < 1 || mem_rows > ((int64_t)1 << 32)))
        return collect_fail(ROVER_ERR_INVALID, fn, ": mem_rows must lie in [1, 2^32]");
    if (reinterpret_cast<uintptr_t>(eps_out) & 15) return collect_fail(ROVER_ERR_INVALID, fn, ": eps_out must be 16-byte aligned");
    const bool vec = ((reinterpret_cast<uintptr_t>(obs_raw) | reinterpret_cast<uintptr_t>(ring_slot_out)) & 15) == 0;
    const size_t units = vec ? total >> 2 : total, per_block = (size_t)REC_THREADS * REC_PER;
    size_t blocks = (units + per_block - 1) / per_block;
    const size_t threads = (size_t)(draws && batch > n ? batch : n);
    if (blocks < (threads + REC_THREADS - 1) / REC_THREADS) blocks = (threads + REC_THREADS - 1) / REC_THREADS;
    if (blocks > 0x7FFFFFFFu) return collect_fail(ROVER_ERR_INVALID, fn, ": n too large");
    Launch R;
    R.rew = rew; R.terminated = terminated; R.rew_out = rew_out; R.term_out = term_out;
    R.ring_pos_entry = ring_pos_entry; R.ring_pos_value = ring_pos_value;
    R.idx_out = idx_out; R.batch = draws ? batch : 0; R.mem_rows = idx_out ? (uint64_t)mem_rows : 1u;
    if constexpr (Launch::DRAWS) R.eps_out = eps_out;
    R.seed_lo = h ? h->seed_lo : 0u; R.seed_hi = h ? h->seed_hi : 0u;
    R.ctr_lo = (uint32_t)(counter & 0xFFFFFFFFu);
    R.ctr_hi = (uint32_t)(counter >> 32);
    if (vec)
        hipLaunchKernelGGL((offpolicy_collect_record_kernel<true, Launch>), dim3((unsigned)blocks), dim3(REC_THREADS), 0,
                           static_cast<hipStream_t>(stream), obs_raw, ring_slot_out, total, n, R);
    else
        hipLaunchKernelGGL((offpolicy_collect_record_kernel<false, Launch>), dim3((unsigned)blocks), dim3(REC_THREADS), 0,
                           static_cast<hipStream_t>(stream), obs_raw, ring_slot_out, total, n, R);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return collect_fail(ROVER_ERR_HIP, fn, "_kernel launch: ", hipGetErrorString(e));
    return ROVER_OK;
}

// the checks every act entry point starts with
inline int collect_act_check(const char *fn, const void *actor, const void *h, const float *packed, const float *obs, const float *act_out,
                             const float *env_act_out, int32_t n, int32_t n_copies)
{
    if (!actor || !h) return collect_fail(ROVER_ERR_INVALID, fn, ": NULL descriptor / hparams");
    if (!packed || !obs || !act_out || !env_act_out) return collect_fail(ROVER_ERR_INVALID, fn, ": NULL required pointer");
    if (n < 1 || n_copies < 1) return collect_fail(ROVER_ERR_INVALID, fn, ": n and n_copies must be >= 1");
    if (reinterpret_cast<uintptr_t>(packed) & 15) return rover_internal_fail(ROVER_ERR_INVALID, "packed weights must be 16-byte aligned");
    return ROVER_OK;
}

// An act kernel (td3_actor_tile's forward and the caller's epilogue) over n rows.  Fills the members every act launch struct starts
// with; the caller has set the rest of L.
template <class Launch>
int collect_act_launch(const char *fn, void (*kernel)(rover_policy_desc, Launch, const float *, const float *, int),
                       const rover_policy_desc *actor, Launch &L, const float *packed, int32_t n_copies, uint64_t counter,
                       const float *obs, int32_t n, void *stream)
{
    L.n_copies = n_copies;
    L.copy_floats = (unsigned)rover_policy_packed_floats(actor);
    L.ctr_lo = (uint32_t)(counter & 0xFFFFFFFFu);
    L.ctr_hi = (uint32_t)(counter >> 32);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(kernel, dim3(ceil_div(n, TDC_ROWS)), dim3(TDC_THREADS), LDS_BYTES, static_cast<hipStream_t>(stream), *actor, L,
                       packed, obs, n);
    e = hipGetLastError();
    if (e != hipSuccess) return collect_fail(ROVER_ERR_HIP, fn, "_kernel launch: ", hipGetErrorString(e));
    return ROVER_OK;
}

}  // namespace

#endif  // ROVER_OFFPOLICY_COLLECT_HPP
