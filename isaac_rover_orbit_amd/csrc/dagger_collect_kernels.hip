// dagger_collect_kernels.hip -- the collector half of a DAgger env step (gfx950 / CDNA4, wave64): the 31 x 31 depth image and the
// env's raw row assembled into a student row of the replay ring, the teacher's label and the student's action from
// td3_actor_tile.hpp's forward (the device function the TD3 and SAC collectors run, bit-identical to rover_policy_forward), the
// counter-based draw and the beta mix.  See include/rover_dagger.h for the contract.
//
//   rover_dagger_rows_kernel  image + env rows -> student rows (and the sanitised env rows the teacher reads); with a record struct
//                             also reward / terminated / ring_pos of the transition and the batch's row indices.  The pixel
//                             rule, the record struct with its host checks and the index stream's tag are
//                             collect_record.hpp's, shared with dagger_conv_kernels.hip
//   rover_dagger_act_kernel   TEACHER: tanh mean -> the label; STUDENT: tanh mean, the draw, the mix -> the env's action.  The mode
//                             is a launch argument and the branch on it is wave-uniform.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_dagger.h"
#include "../../include/rover_hip.h"
#include "../../include/rover_td3_explore.h"
#include "offpolicy_collect.hpp"
#include "rover_internal.hpp"
#include "td3_actor_tile.hpp"
#include "train_math.hpp"

namespace {

constexpr int PIX = 961;                      // 31 x 31 pixels = OBS - PROP
constexpr int ROWS_THREADS = 256;             // rows kernel: one 16-byte piece of the output per thread
enum { DAGGER_TEACHER = 0, DAGGER_STUDENT = 1 };

// VEC: every pointer is 16-byte aligned.  Thread gid owns floats [4 gid, 4 gid + 4) of the output, which is `total` = n * 965
// floats.  Output float 965 r + 4 + p and depth float 961 r + p lie 4 r + 4 floats apart: an aligned output piece inside one row's
// pixel columns is an aligned piece of the image.  The grid also covers n and batch threads for the record and the indices.
template <bool VEC>
__global__ __launch_bounds__(ROWS_THREADS) void rover_dagger_rows_kernel(const float *__restrict__ depth, const float *__restrict__ env,
                                                                         float *__restrict__ out, float *__restrict__ teacher,
                                                                         size_t total, int n, float clip, float scale, RecFields R)
{
    const size_t gid = (size_t)blockIdx.x * ROWS_THREADS + threadIdx.x;
    const size_t g0 = 4 * gid;
    if (g0 < total) {
        const size_t r0 = g0 / OBS;
        const int c0 = (int)(g0 - r0 * OBS);
        if (VEC && c0 >= PROP && c0 + 3 < OBS) {
            const v4f d = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(depth + (g0 - 4 * r0 - 4)));   // read once
            v4f s;
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] = depth_value(d[j], clip, scale);
            *reinterpret_cast<v4f *>(out + g0) = s;       // a plain store: the next act launch reads this slot
            if (teacher) {
                const v4f e = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(env + g0));
                v4f t;
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = sanitise(e[j]);
                *reinterpret_cast<v4f *>(teacher + g0) = t;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t g = g0 + j;
                if (g >= total) break;
                const size_t r = g / OBS;
                const int c = (int)(g - r * OBS);
                if (c < PROP || teacher) {
                    const float e = sanitise(env[g]);
                    if (teacher) teacher[g] = e;
                    if (c < PROP) out[g] = e;
                }
                if (c >= PROP) out[g] = depth_value(depth[r * PIX + (c - PROP)], clip, scale);
            }
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
        const uint32_t w = (gid & 2) ? ((gid & 1) ? w4[3] : w4[2]) : ((gid & 1) ? w4[1] : w4[0]);   // selects, not a private array
        R.idx_out[gid] = (int64_t)(((uint64_t)w * R.mem_rows) >> 32);   // mem_rows <= 2^32: the product fits 64 bits
    }
}

struct DaggerActLaunch {
    int n_copies;              // replicas of the packed buffer; workgroup b reads replica b % n_copies
    unsigned copy_floats;
    uint32_t ctr_lo, ctr_hi;
    uint32_t seed_lo, seed_hi, id0;
    int mode;
    float beta;
    const float *label_in;     // STUDENT: the labels the TEACHER launch wrote
    float *label_out;          // TEACHER
    float *env_act_out, *student_out;
    uint8_t *source_out;
};

__global__ __launch_bounds__(TDC_THREADS) void rover_dagger_act_kernel(rover_policy_desc d, DaggerActLaunch L,
                                                                       const float *__restrict__ packed, const float *__restrict__ obs, int n)
{
    extern __shared__ __align__(16) float lds[];
    Td3ActorLane p;
    if (!td3_actor_tile(d, packed, L.n_copies, L.copy_floats, obs, n, lds, p)) return;
    const float a = rv_tanhf(p.y);
    if (L.mode == DAGGER_TEACHER) {
        if (p.live) L.label_out[p.o] = a;
        return;
    }
    // column 0 of the TD3 explorer's random steps (rover_td3_explore.h); the two lanes of a row repeat the row's Philox block
    uint32_t w4[4];
    philox4x32(L.id0 + (uint32_t)p.row, L.ctr_lo, L.ctr_hi, ROVER_TD3_TAG_RANDOM | 0u, L.seed_lo, L.seed_hi, w4);
    const float u = unit_uniform(w4[0]);
    const bool from_teacher = u < L.beta;
    if (p.live) {
        if (L.student_out) L.student_out[p.o] = a;
        L.env_act_out[p.o] = from_teacher ? L.label_in[p.o] : a;
        if (L.source_out && p.c == 0) L.source_out[p.row] = from_teacher ? 1 : 0;
    }
}

// rover_dagger_rows and rover_dagger_record: argument checks, the vector / scalar choice, the grid and the launch
int rows_launch(const char *fn, const rover_dagger_hparams *h, const float *depth, const float *env_raw, int32_t n, float *rows_out,
                float *teacher_rows_out, const float *rew, const uint8_t *terminated, float *rew_out, uint8_t *term_out,
                int32_t *ring_pos_entry, int32_t ring_pos_value, int64_t *idx_out, int32_t batch, int64_t mem_rows, uint64_t counter,
                void *stream)
{
    if (!h) return collect_fail(ROVER_ERR_INVALID, fn, ": hparams is NULL");
    if (!depth || !env_raw || !rows_out) return collect_fail(ROVER_ERR_INVALID, fn, ": NULL rows");
    if (n < 1) return collect_fail(ROVER_ERR_INVALID, fn, ": n must be >= 1");
    if (!(h->depth_clip > 0.0f) || !(h->depth_clip < INFINITY) || !(h->depth_scale == h->depth_scale))
        return collect_fail(ROVER_ERR_INVALID, fn, ": depth_clip must be positive and finite, depth_scale a number");
    const size_t total = (size_t)n * OBS, bytes = total * sizeof(float), dbytes = (size_t)n * PIX * sizeof(float);
    if (overlap(rows_out, bytes, env_raw, bytes) || overlap(rows_out, bytes, depth, dbytes) ||
        (teacher_rows_out && (overlap(teacher_rows_out, bytes, env_raw, bytes) || overlap(teacher_rows_out, bytes, depth, dbytes) ||
                              overlap(teacher_rows_out, bytes, rows_out, bytes))))
        return collect_fail(ROVER_ERR_INVALID, fn, ": the outputs must not alias the inputs or each other");
    if (int rc = rec_check(fn, rew, terminated, rew_out, term_out, idx_out, batch, mem_rows)) return rc;
    const bool vec = ((reinterpret_cast<uintptr_t>(depth) | reinterpret_cast<uintptr_t>(env_raw) | reinterpret_cast<uintptr_t>(rows_out) |
                       reinterpret_cast<uintptr_t>(teacher_rows_out)) & 15) == 0;
    size_t threads = (total + 3) >> 2;
    if (threads < (size_t)n) threads = (size_t)n;
    if (idx_out && threads < (size_t)batch) threads = (size_t)batch;
    const size_t blocks = (threads + ROWS_THREADS - 1) / ROWS_THREADS;
    if (blocks > 0x7FFFFFFFu) return collect_fail(ROVER_ERR_INVALID, fn, ": n too large");
    const RecFields R = rec_fill(h, counter, rew, terminated, rew_out, term_out, ring_pos_entry, ring_pos_value, idx_out, batch, mem_rows);
    if (vec)
        hipLaunchKernelGGL(rover_dagger_rows_kernel<true>, dim3((unsigned)blocks), dim3(ROWS_THREADS), 0, static_cast<hipStream_t>(stream),
                           depth, env_raw, rows_out, teacher_rows_out, total, n, h->depth_clip, h->depth_scale, R);
    else
        hipLaunchKernelGGL(rover_dagger_rows_kernel<false>, dim3((unsigned)blocks), dim3(ROWS_THREADS), 0, static_cast<hipStream_t>(stream),
                           depth, env_raw, rows_out, teacher_rows_out, total, n, h->depth_clip, h->depth_scale, R);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return collect_fail(ROVER_ERR_HIP, fn, "_kernel launch: ", hipGetErrorString(e));
    return ROVER_OK;
}

}  // namespace

extern "C" {

int rover_dagger_rows(const rover_dagger_hparams *h, const float *depth, const float *env_raw, int32_t n, float *rows_out,
                      float *teacher_rows_out, void *stream)
{
    return rows_launch("rover_dagger_rows", h, depth, env_raw, n, rows_out, teacher_rows_out, nullptr, nullptr, nullptr, nullptr, nullptr,
                       0, nullptr, 0, 0, 0, stream);
}

int rover_dagger_record(const rover_dagger_hparams *h, const float *depth, const float *env_raw, int32_t n, float *ring_slot_out,
                        float *teacher_rows_out, const float *rew, const uint8_t *terminated, float *rew_out, uint8_t *term_out,
                        int32_t *ring_pos_entry, int32_t ring_pos_value, int64_t *idx_out, int32_t batch, int64_t mem_rows,
                        uint64_t counter, void *stream)
{
    return rows_launch("rover_dagger_record", h, depth, env_raw, n, ring_slot_out, teacher_rows_out, rew, terminated, rew_out, term_out,
                       ring_pos_entry, ring_pos_value, idx_out, batch, mem_rows, counter, stream);
}

int rover_dagger_act(const rover_policy_desc *teacher, const float *teacher_packed, int32_t teacher_copies,
                     const rover_policy_desc *student, const float *student_packed, int32_t student_copies,
                     const rover_dagger_hparams *h, uint64_t counter, float beta, const float *teacher_rows,
                     const float *student_rows, int32_t n, float *label_out, float *env_act_out, float *student_out,
                     uint8_t *source_out, void *stream)
{
    const char *fn = "rover_dagger_act";
    if (int rc = collect_act_check(fn, teacher, h, teacher_packed, teacher_rows, label_out, env_act_out, n, teacher_copies)) return rc;
    if (int rc = collect_act_check(fn, student, h, student_packed, student_rows, label_out, env_act_out, n, student_copies)) return rc;
    if (!(beta >= 0.0f && beta <= 1.0f)) return collect_fail(ROVER_ERR_INVALID, fn, ": beta must lie in [0, 1]");
    for (const rover_policy_desc *d : {teacher, student})
        if (!is_reference_actor(d, ROVER_ACT_TANH) || d->layers[5].N != 2)
            return collect_fail(ROVER_ERR_UNSUPPORTED, fn, ": teacher and student must have the reference architecture with two tanh outputs");
    if (overlap(label_out, (size_t)n * 2 * sizeof(float), env_act_out, (size_t)n * 2 * sizeof(float)))
        return collect_fail(ROVER_ERR_INVALID, fn, ": label_out must not alias env_act_out");
    DaggerActLaunch L = {};
    L.seed_lo = h->seed_lo; L.seed_hi = h->seed_hi; L.id0 = (uint32_t)h->env_id_offset;
    L.beta = beta;
    L.mode = DAGGER_TEACHER;
    L.label_out = label_out;
    if (int rc = collect_act_launch(fn, rover_dagger_act_kernel, teacher, L, teacher_packed, teacher_copies, counter, teacher_rows, n, stream))
        return rc;
    L.mode = DAGGER_STUDENT;
    L.label_in = label_out; L.label_out = nullptr;
    L.env_act_out = env_act_out; L.student_out = student_out; L.source_out = source_out;
    return collect_act_launch(fn, rover_dagger_act_kernel, student, L, student_packed, student_copies, counter, student_rows, n, stream);
}

}  // extern "C"
