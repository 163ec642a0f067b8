// trace_kernels.hip -- the device-side episode recorder (gfx950 / CDNA4, wave64): per env step one launch that stages every
// stream's rows into per-env rings and one single-workgroup launch that commits the finished episodes, in env-id order, to a
// descriptor list; per drain a gather that packs the committed episodes, in list order, into output blocks.  See
// include/rover_trace.h for the contract.
//
// Work is cut into wave items.  A WIDE stream (row_bytes > 16) gives one wave a span of at most SPAN bytes of one row: the wave's
// row, ring slot and span are wave-uniform, its lanes move 16-byte pieces when both ends are 16-byte aligned, 4-byte loads packed
// into 16-byte stores (or the reverse) when one end is only 4-byte aligned, 4-byte pieces when both are, bytes otherwise.  A
// NARROW stream (rewards, flags, small extras) gives one lane a whole row, 64 rows per wave.  Nothing here communicates between
// workgroups inside a launch: the append kernel only READS head / len / pending, the commit kernel (one workgroup) is their only
// writer, and the launch boundary orders the two.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/rover_hip.h"
#include "../../include/rover_trace.h"
#include "rover_internal.hpp"

namespace {

constexpr int TR_THREADS = 256;                    // 4 waves
constexpr int TR_WAVES = TR_THREADS / 64;
constexpr int SPAN = 4096;                         // bytes of a wide row one wave moves: 64 lanes x 16 bytes x 4
constexpr int NARROW = 16;                         // rows up to this many bytes are moved one per lane
constexpr int HDR = ROVER_TRACE_HEADER_WORDS;
constexpr int CHUNK = ROVER_TRACE_COMMIT_CHUNK;    // = the commit kernel's workgroup
constexpr int W_COUNT = 0, W_STATUS = 1, W_ROWS = 2;

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef int32_t v4i __attribute__((ext_vector_type(4)));

__host__ __device__ inline int desc_word(int n) { return HDR + ((3 * n + 3) & ~3); }   // 16-byte aligned descriptors

struct TrStream {
    const uint8_t *src;     // append: the caller's rows; gather: unused
    uint8_t *stage;
    uint8_t *out;
    int64_t src_pitch, stage_pitch, out_pitch;
    int32_t row_bytes, flags;
    int32_t spans;          // wave items per row; 0: narrow (one lane per row)
    int32_t first;          // index of the stream's first wave item
};

struct TrPlan {
    TrStream s[ROVER_TRACE_MAX_STREAMS];
    int32_t n_streams, items;
};

// `len` bytes from s to d by the 64 lanes of a wave.  The two ranges never overlap (caller's rows / stage / output blocks).
__device__ __forceinline__ void copy_span(const uint8_t *__restrict__ s, uint8_t *__restrict__ d, int len, int lane)
{
    const uintptr_t sa = reinterpret_cast<uintptr_t>(s), da = reinterpret_cast<uintptr_t>(d);
    int moved = 0;
    if (((sa | da) & 3) == 0) {
        const uint32_t *s32 = reinterpret_cast<const uint32_t *>(s);
        uint32_t *d32 = reinterpret_cast<uint32_t *>(d);
        const bool s16 = (sa & 15) == 0, d16 = (da & 15) == 0;
        const int n16 = len >> 4;
        if (s16 && d16) {
#pragma unroll 4
            for (int i = lane; i < n16; i += 64) reinterpret_cast<v4u *>(d)[i] = reinterpret_cast<const v4u *>(s)[i];
            moved = n16 << 4;
        } else if (d16) {                           // e.g. an observation row (3860-byte stride) into its padded stage row
#pragma unroll 4
            for (int i = lane; i < n16; i += 64) {
                const uint32_t *p = s32 + 4 * i;
                const v4u v = {p[0], p[1], p[2], p[3]};
                reinterpret_cast<v4u *>(d)[i] = v;
            }
            moved = n16 << 4;
        } else if (s16) {                           // e.g. a padded stage row into a packed output block
#pragma unroll 4
            for (int i = lane; i < n16; i += 64) {
                const v4u v = reinterpret_cast<const v4u *>(s)[i];
                uint32_t *q = d32 + 4 * i;
                q[0] = v[0]; q[1] = v[1]; q[2] = v[2]; q[3] = v[3];
            }
            moved = n16 << 4;
        }
        const int n4 = len >> 2;
        for (int i = (moved >> 2) + lane; i < n4; i += 64) d32[i] = s32[i];
        moved = n4 << 2;
    }
    for (int i = moved + lane; i < len; i += 64) d[i] = s[i];
}

// one whole narrow row by one lane
__device__ __forceinline__ void copy_row(const uint8_t *__restrict__ s, uint8_t *__restrict__ d, int len, int flags)
{
    if (flags & ROVER_TRACE_BOOL) {
        for (int i = 0; i < len; ++i) d[i] = s[i] != 0 ? 1 : 0;
    } else if (((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d) | (uintptr_t)len) & 3) == 0) {
        for (int i = 0; i < (len >> 2); ++i) reinterpret_cast<uint32_t *>(d)[i] = reinterpret_cast<const uint32_t *>(s)[i];
    } else {
        for (int i = 0; i < len; ++i) d[i] = s[i];
    }
}

// the stream a wave item belongs to (items are numbered stream by stream; at most 16 streams)
__device__ __forceinline__ int find_stream(const TrPlan &P, int item)
{
    int k = 0;
    for (int j = 1; j < P.n_streams; ++j)
        if (item >= P.s[j].first) k = j;
    return k;
}

__global__ __launch_bounds__(TR_THREADS) void rover_trace_append_kernel(TrPlan P, const int32_t *state, int n, int R, int max_ep)
{
    const int lane = threadIdx.x & 63;
    const int item = __builtin_amdgcn_readfirstlane((int)blockIdx.x * TR_WAVES + ((int)threadIdx.x >> 6));
    if (item >= P.items) return;
    const int32_t *head = state + HDR, *len = head + n, *pend = len + n;
    const int k = find_stream(P, item);
    const TrStream &S = P.s[k];
    const int local = item - S.first;
    if (S.spans == 0) {
        const int e = local * 64 + lane;
        if (e >= n) return;
        const int l = len[e];
        if (l >= max_ep || pend[e] + l >= R) return;                       // the commit kernel raises the status
        const int slot = (head[e] + l) % R;
        copy_row(S.src + (size_t)e * S.src_pitch, S.stage + ((size_t)e * R + slot) * S.stage_pitch, S.row_bytes, S.flags);
    } else {
        const int e = local / S.spans, c = local - e * S.spans;
        const int l = len[e];
        if (l >= max_ep || pend[e] + l >= R) return;
        const int slot = (head[e] + l) % R;
        const int o = c * SPAN;
        copy_span(S.src + (size_t)e * S.src_pitch + o, S.stage + ((size_t)e * R + slot) * S.stage_pitch + o, min(SPAN, S.row_bytes - o),
                  lane);
    }
}

// One workgroup.  Envs are visited CHUNK at a time in id order; inside a chunk the descriptor index and the row offset of a done
// env are the exclusive prefix sums over the chunk's done envs (ballot + shuffles inside a wave, LDS across the four waves), and
// the carry into the next chunk is the running count / row total.
__global__ __launch_bounds__(CHUNK) void rover_trace_commit_kernel(int32_t *state, int n, int R, int max_ep, int cap,
                                                                    const uint8_t *__restrict__ done, int all)
{
    __shared__ int wave_c[CHUNK / 64], wave_r[CHUNK / 64], raised;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t *head = state + HDR, *len = head + n, *pend = len + n;
    v4i *desc = reinterpret_cast<v4i *>(state + desc_word(n));
    if (tid == 0) raised = 0;
    int count = state[W_COUNT], total = state[W_ROWS], flags = 0;
    __syncthreads();                                 // every thread has read the header; `raised` is initialised
    for (int base = 0; base < n; base += CHUNK) {
        const int e = base + tid;
        const bool valid = e < n;
        int h = 0, l = 0, p = 0;
        bool emit = false;
        if (valid) {
            h = head[e]; l = len[e]; p = pend[e];
            if (!all) {
                if (l >= max_ep) flags |= ROVER_TRACE_ST_EPISODE;
                else if (p + l >= R) flags |= ROVER_TRACE_ST_RING;
                else l += 1;                         // the row the append launch staged
            }
            emit = (all || done[e] != 0) && l > 0;
        }
        const int rows = emit ? l : 0;
        const unsigned long long ballot = __ballot(emit);
        const int c_excl = __popcll(ballot & ((1ull << lane) - 1ull));
        int r_incl = rows;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(r_incl, d, 64);
            if (lane >= d) r_incl += v;
        }
        if (lane == 63) {
            wave_c[wave] = __popcll(ballot);
            wave_r[wave] = r_incl;
        }
        __syncthreads();
        int c_off = 0, r_off = 0, c_all = 0, r_all = 0;
#pragma unroll
        for (int w = 0; w < CHUNK / 64; ++w) {
            if (w < wave) { c_off += wave_c[w]; r_off += wave_r[w]; }
            c_all += wave_c[w];
            r_all += wave_r[w];
        }
        if (valid) {
            if (emit) {
                const int idx = count + c_off + c_excl;
                if (idx < cap) desc[idx] = (v4i){e, h, l, total + r_off + (r_incl - rows)};
                else flags |= ROVER_TRACE_ST_DESC;
                head[e] = (h + l) % R;
                len[e] = 0;
                pend[e] = p + l;
            } else {
                len[e] = l;
            }
        }
        count += c_all;
        total += r_all;
        __syncthreads();                             // wave_c / wave_r are rewritten by the next chunk
    }
    if (flags) atomicOr(&raised, flags);
    __syncthreads();
    if (tid == 0) {
        state[W_COUNT] = count;
        state[W_ROWS] = total;
        if (raised) state[W_STATUS] |= raised;
    }
}

__global__ __launch_bounds__(TR_THREADS) void rover_trace_gather_kernel(TrPlan P, const int32_t *state, int n, int R, int cap, int r0,
                                                                        int rows)
{
    const int lane = threadIdx.x & 63;
    const int item = __builtin_amdgcn_readfirstlane((int)blockIdx.x * TR_WAVES + ((int)threadIdx.x >> 6));
    if (item >= P.items) return;
    const int total = state[W_ROWS], cnt = min(state[W_COUNT], cap);
    if (cnt < 1) return;
    const v4i *desc = reinterpret_cast<const v4i *>(state + desc_word(n));
    const int k = find_stream(P, item);
    const TrStream &S = P.s[k];
    const int local = item - S.first;
    const bool narrow = S.spans == 0;
    const int i = narrow ? local * 64 + lane : local / S.spans;             // output row of this lane / wave
    const int r = r0 + i;
    if (i >= rows || r >= total) return;
    int lo = 0, hi = cnt;                                                   // the last descriptor with offset <= r
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (desc[mid][3] <= r) lo = mid;
        else hi = mid;
    }
    const v4i d = desc[lo];
    const int env = min(max(d[0], 0), n - 1);
    const int slot = (int)((unsigned)(d[1] + (r - d[3])) % (unsigned)R);
    const uint8_t *s = S.stage + ((size_t)env * R + slot) * S.stage_pitch;
    uint8_t *o = S.out + (size_t)i * S.out_pitch;
    if (narrow) {
        copy_row(s, o, S.row_bytes, 0);                                     // the flag was applied when the row was staged
    } else {
        const int c = local - i * S.spans, off = c * SPAN;
        copy_span(s + off, o + off, min(SPAN, S.row_bytes - off), lane);
    }
}

__global__ __launch_bounds__(TR_THREADS) void rover_trace_drained_kernel(int32_t *state, int n)
{
    const int e = blockIdx.x * TR_THREADS + threadIdx.x;
    if (e < n) state[HDR + 2 * n + e] = 0;
    if (e == 0) {
        state[W_COUNT] = 0;
        state[W_ROWS] = 0;
    }
}

size_t stage_pitch(int32_t row_bytes)
{
    if (row_bytes <= 0) return 0;
    const size_t a = row_bytes >= 16 ? 16 : 4;
    return ((size_t)row_bytes + a - 1) / a * a;
}

// argument checks shared by append and gather; fills the plan for `m` rows per stream
int make_plan(const char *who, const rover_trace_stream *streams, int32_t n_streams, bool gather, int64_t m, TrPlan *P)
{
    if (!streams) return rover_internal_fail(ROVER_ERR_INVALID, "%s: streams is NULL", who);
    if (n_streams < 1 || n_streams > ROVER_TRACE_MAX_STREAMS)
        return rover_internal_fail(ROVER_ERR_INVALID, "%s: n_streams must lie in [1, ROVER_TRACE_MAX_STREAMS]", who);
    int64_t items = 0;
    for (int k = 0; k < n_streams; ++k) {
        const rover_trace_stream &u = streams[k];
        if (u.row_bytes <= 0) return rover_internal_fail(ROVER_ERR_INVALID, "%s: row_bytes must be > 0", who);
        if (!u.stage || (gather ? !u.out : !u.src)) return rover_internal_fail(ROVER_ERR_INVALID, "%s: NULL stream pointer", who);
        if (u.stage_pitch < u.row_bytes || (gather ? u.out_pitch < u.row_bytes : u.src_pitch < u.row_bytes))
            return rover_internal_fail(ROVER_ERR_INVALID, "%s: a pitch is smaller than row_bytes", who);
        if (u.flags & ~ROVER_TRACE_BOOL) return rover_internal_fail(ROVER_ERR_INVALID, "%s: unknown stream flag", who);
        if ((u.flags & ROVER_TRACE_BOOL) && u.row_bytes > NARROW)
            return rover_internal_fail(ROVER_ERR_INVALID, "%s: ROVER_TRACE_BOOL needs row_bytes <= 16", who);
        TrStream &t = P->s[k];
        t.src = static_cast<const uint8_t *>(u.src);
        t.stage = static_cast<uint8_t *>(u.stage);
        t.out = static_cast<uint8_t *>(u.out);
        t.src_pitch = u.src_pitch; t.stage_pitch = u.stage_pitch; t.out_pitch = u.out_pitch;
        t.row_bytes = u.row_bytes; t.flags = u.flags;
        t.spans = u.row_bytes <= NARROW ? 0 : (u.row_bytes + SPAN - 1) / SPAN;
        t.first = (int32_t)items;
        items += t.spans == 0 ? (m + 63) / 64 : m * t.spans;
        if (items > 0x3FFFFFFF) return rover_internal_fail(ROVER_ERR_INVALID, "%s: too many rows for one launch", who);
    }
    for (int k = n_streams; k < ROVER_TRACE_MAX_STREAMS; ++k) memset(&P->s[k], 0, sizeof(TrStream));
    P->n_streams = n_streams;
    P->items = (int32_t)items;
    return ROVER_OK;
}

int check_layout(const char *who, const int32_t *state, int32_t n, int32_t R, int32_t desc_cap)
{
    if (!state) return rover_internal_fail(ROVER_ERR_INVALID, "%s: state is NULL", who);
    if (reinterpret_cast<uintptr_t>(state) & 15) return rover_internal_fail(ROVER_ERR_INVALID, "%s: state must be 16-byte aligned", who);
    if (n <= 0) return rover_internal_fail(ROVER_ERR_INVALID, "%s: n must be > 0", who);
    if (R < 2) return rover_internal_fail(ROVER_ERR_INVALID, "%s: R must be >= max_episode_rows + 1", who);
    if ((int64_t)n * R > 0x7FFFFFFF) return rover_internal_fail(ROVER_ERR_INVALID, "%s: n * R must stay below 2^31", who);
    if (desc_cap <= 0) return rover_internal_fail(ROVER_ERR_INVALID, "%s: desc_cap must be > 0", who);
    return ROVER_OK;
}

}  // namespace

extern "C" {

size_t rover_trace_stream_bytes(void) { return sizeof(rover_trace_stream); }

size_t rover_trace_stage_pitch(int32_t row_bytes) { return stage_pitch(row_bytes); }

size_t rover_trace_stage_bytes(int32_t n, int32_t R, int32_t row_bytes)
{
    if (n <= 0 || R <= 0 || row_bytes <= 0) return 0;
    return (size_t)n * (size_t)R * stage_pitch(row_bytes);
}

size_t rover_trace_state_bytes(int32_t n, int32_t desc_cap)
{
    if (n <= 0 || desc_cap <= 0) return 0;
    return sizeof(int32_t) * ((size_t)desc_word(n) + 4 * (size_t)desc_cap);
}

int rover_trace_init(int32_t *state, int32_t n, int32_t desc_cap, void *stream)
{
    if (!state || n <= 0 || desc_cap <= 0) return rover_internal_fail(ROVER_ERR_INVALID, "rover_trace_init: NULL state, n <= 0 or desc_cap <= 0");
    if (reinterpret_cast<uintptr_t>(state) & 15) return rover_internal_fail(ROVER_ERR_INVALID, "rover_trace_init: state must be 16-byte aligned");
    const hipError_t e = hipMemsetAsync(state, 0, rover_trace_state_bytes(n, desc_cap), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "rover_trace_init: hipMemsetAsync: %s", hipGetErrorString(e));
    return ROVER_OK;
}

int rover_trace_append(const rover_trace_stream *streams, int32_t n_streams, int32_t *state, int32_t n, int32_t R,
                       int32_t max_episode_rows, int32_t desc_cap, const uint8_t *done, void *stream)
{
    int rc = check_layout("rover_trace_append", state, n, R, desc_cap);
    if (rc) return rc;
    if (!done) return rover_internal_fail(ROVER_ERR_INVALID, "rover_trace_append: done is NULL");
    if (max_episode_rows < 1 || R < (int64_t)max_episode_rows + 1)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_trace_append: needs max_episode_rows >= 1 and R >= max_episode_rows + 1");
    TrPlan P;
    rc = make_plan("rover_trace_append", streams, n_streams, false, n, &P);
    if (rc) return rc;
    hipLaunchKernelGGL(rover_trace_append_kernel, dim3((P.items + TR_WAVES - 1) / TR_WAVES), dim3(TR_THREADS), 0,
                       static_cast<hipStream_t>(stream), P, state, n, R, max_episode_rows);
    rc = launched("rover_trace_append_kernel launch: %s");
    if (rc) return rc;
    hipLaunchKernelGGL(rover_trace_commit_kernel, dim3(1), dim3(CHUNK), 0, static_cast<hipStream_t>(stream), state, n, R,
                       max_episode_rows, desc_cap, done, 0);
    return launched("rover_trace_commit_kernel launch: %s");
}

int rover_trace_commit_all(int32_t *state, int32_t n, int32_t R, int32_t desc_cap, void *stream)
{
    const int rc = check_layout("rover_trace_commit_all", state, n, R, desc_cap);
    if (rc) return rc;
    hipLaunchKernelGGL(rover_trace_commit_kernel, dim3(1), dim3(CHUNK), 0, static_cast<hipStream_t>(stream), state, n, R, 0x7FFFFFFF,
                       desc_cap, static_cast<const uint8_t *>(nullptr), 1);
    return launched("rover_trace_commit_kernel launch: %s");
}

int rover_trace_gather(const rover_trace_stream *streams, int32_t n_streams, const int32_t *state, int32_t n, int32_t R, int32_t desc_cap,
                       int32_t r0, int32_t rows, void *stream)
{
    int rc = check_layout("rover_trace_gather", state, n, R, desc_cap);
    if (rc) return rc;
    if (r0 < 0 || rows < 1 || (int64_t)r0 + rows > 0x7FFFFFFF)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_trace_gather: needs r0 >= 0, rows >= 1 and r0 + rows < 2^31");
    TrPlan P;
    rc = make_plan("rover_trace_gather", streams, n_streams, true, rows, &P);
    if (rc) return rc;
    hipLaunchKernelGGL(rover_trace_gather_kernel, dim3((P.items + TR_WAVES - 1) / TR_WAVES), dim3(TR_THREADS), 0,
                       static_cast<hipStream_t>(stream), P, state, n, R, desc_cap, r0, rows);
    return launched("rover_trace_gather_kernel launch: %s");
}

int rover_trace_drained(int32_t *state, int32_t n, void *stream)
{
    if (!state || n <= 0) return rover_internal_fail(ROVER_ERR_INVALID, "rover_trace_drained: NULL state or n <= 0");
    hipLaunchKernelGGL(rover_trace_drained_kernel, dim3((n + TR_THREADS - 1) / TR_THREADS), dim3(TR_THREADS), 0,
                       static_cast<hipStream_t>(stream), state, n);
    return launched("rover_trace_drained_kernel launch: %s");
}

}  // extern "C"
