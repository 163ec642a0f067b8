// dagger_conv_kernels.hip -- fused DAgger at the camera's native 160 x 90: the learned convolutional stem in front of the
// reference network (gfx950 / CDNA4, wave64).  See include/rover_dagger_conv.h for the contract, the accumulation order of a
// feature and the reduction orders.
//
//   rover_dagger_conv_rows_kernel    collector: one workgroup per env.  The depth image becomes x (clip, scale), goes to the image
//                                    ring and to LDS; the stem runs from LDS into the ring slot's feature columns; the env row is
//                                    sanitised into the slot's first four columns and the teacher's rows; one launch also does the
//                                    record's bookkeeping (reward, terminated, ring_pos, the batch's indices)
//   dagger_conv_forward_kernel       update: one workgroup per sampled row, the same stem from the image ring into a gathered row
//   dagger_conv_backward_kernel      update: one workgroup per chunk of 8 sampled rows; recomputes the pre-activations, sums
//                                    db2 / dw2 / db1 per thread and dW1 = dpre^T im2col(x) on v_mfma_f32_16x16x4_f32
//   dagger_head / norm / final / adam_kernel   dagger_tail.hpp's loss head and optimiser tail, shared with dagger_kernels.hip: Adam
//                                    over the vector [head | stem], the replicas of the head alone
//
// The record struct with its host checks, the pixel rule depth_value() and the index stream's tag are collect_record.hpp's,
// shared with dagger_collect_kernels.hip and the off-policy collectors.
//
// stem_feature() is the ONE device function that forms a feature (stem_pre() is its first half, which the backward calls for the
// pre-activations): every kernel agrees on the bits.  The network's forward, backward, weight gradients, the input gradient (the
// backward kernel without an activation reference) and the chunk combine are offpolicy_net.hpp's, as they stand.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_dagger_conv.h"
#include "../../include/rover_hip.h"
#include "../../include/rover_policy.h"
#include "rover_internal.hpp"
#include "offpolicy_net.hpp"
#include "train_math.hpp"
#include "dagger_tail.hpp"

namespace {

constexpr int IH = ROVER_DAGGER_CONV_IMG_H, IW = ROVER_DAGGER_CONV_IMG_W, PIXN = ROVER_DAGGER_CONV_PIXELS;
constexpr int FS = 31, FEAT = FS * FS;                       // 31 x 31 features = OBS - PROP
constexpr int KH = 6, KW = 10, SH = 3, SW = 5, PADH = 3;     // kernel, stride, rows of zero padding above and below
constexpr int CCH = 8, TAPS = KH * KW;                       // channels; taps of one window
constexpr int O_W1 = 0, O_B1 = CCH * TAPS, O_W2 = O_B1 + CCH, O_B2 = O_W2 + CCH;   // offsets inside the 497 floats
constexpr int STEM_F = ROVER_DAGGER_CONV_STEM_FLOATS, STEM_PAD = 512;
constexpr int ST = 512, SWAVES = ST / 64;                    // threads and waves of the three stem kernels
constexpr int XS_F = (IH + 2 * PADH) * IW;                   // the x image in LDS with its zero rows: 96 x 160 floats = 61440 B
constexpr int RC = 8;                                        // sampled rows per workgroup of the backward
constexpr int DPP = 68;                                      // pitch of a wave's dpre rows in LDS: lanes (c, k) hit banks 4 c + k
constexpr int NSUM = 2 * CCH + 1;                            // db1[8], dw2[8], db2
static_assert(O_B2 + 1 == STEM_F && FEAT + PROP == OBS && PIXN == IH * IW, "stem layout");
static_assert(PIXN / 4 == 7 * ST + 16, "stage_image's load plan");
static_assert(SWAVES * 2 * 64 >= FEAT, "two groups of 64 outputs per wave cover the features");

// The image of one env into LDS rows 3 .. 92 of xs (rows 0 .. 2 and 93 .. 95 are the zero padding), 16 bytes per lane per load,
// all of a thread's loads in flight before the first use.  RAW: src holds metres; x = depth_value() also goes to img_out (the
// image ring).  Otherwise src holds x already.  Ends with a barrier.
template <bool RAW>
__device__ __forceinline__ void stage_image(const float *__restrict__ src, float *xs, float *__restrict__ img_out, float clip, float scale)
{
    const int tid = threadIdx.x;
    const v4f *s4 = reinterpret_cast<const v4f *>(src);
    v4f d[8];
#pragma unroll
    for (int k = 0; k < 7; ++k) d[k] = RAW ? __builtin_nontemporal_load(s4 + tid + k * ST) : s4[tid + k * ST];
    d[7] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    if (tid < 16) d[7] = RAW ? __builtin_nontemporal_load(s4 + tid + 7 * ST) : s4[tid + 7 * ST];
    if (tid < PADH * IW) {
        xs[tid] = 0.0f;
        xs[(PADH + IH) * IW + tid] = 0.0f;
    }
    v4f *x4 = reinterpret_cast<v4f *>(xs + PADH * IW);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k == 7 && tid >= 16) break;
        v4f x = d[k];
        if (RAW) {
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = depth_value(x[j], clip, scale);
            reinterpret_cast<v4f *>(img_out)[tid + k * ST] = x;
        }
        x4[tid + k * ST] = x;
    }
    __syncthreads();
}

// the eight pre-activations of feature (i, j) from the LDS image: acc_c = fma(W1[c][u][v], x, acc_c) over u, then v, ascending,
// then + b1[c].  The parameters are read at uniform addresses (scalar loads); neighbouring j read LDS words 5 apart.
__device__ __forceinline__ void stem_pre(const float *xs, const float *__restrict__ prm, int i, int j, float pre[CCH])
{
    const float *w = xs + (SH * i) * IW + SW * j;
    float acc[CCH];
#pragma unroll
    for (int c = 0; c < CCH; ++c) acc[c] = 0.0f;
#pragma unroll 1
    for (int u = 0; u < KH; ++u)                              // one kernel row per trip: its 80 weights fit the scalar registers
#pragma unroll
        for (int v = 0; v < KW; ++v) {
            const float x = w[u * IW + v];
#pragma unroll
            for (int c = 0; c < CCH; ++c) acc[c] = __builtin_fmaf(prm[O_W1 + c * TAPS + u * KW + v], x, acc[c]);
        }
#pragma unroll
    for (int c = 0; c < CCH; ++c) pre[c] = acc[c] + prm[O_B1 + c];
}

// THE feature: y = b2, then y = fma(w2[c], leaky(pre_c), y) for c ascending
__device__ __forceinline__ float stem_feature(const float *xs, const float *__restrict__ prm, int i, int j)
{
    float pre[CCH];
    stem_pre(xs, prm, i, j, pre);
    float y = prm[O_B2];
#pragma unroll
    for (int c = 0; c < CCH; ++c) y = __builtin_fmaf(prm[O_W2 + c], leaky(pre[c], 0.01f), y);
    return y;
}

// ---- collector
__global__ __launch_bounds__(ST) void rover_dagger_conv_rows_kernel(const float *__restrict__ prm, const float *__restrict__ depth,
                                                                    const float *__restrict__ env, float *__restrict__ slot,
                                                                    float *__restrict__ img, float *__restrict__ teacher, int n,
                                                                    float clip, float scale, RecFields R)
{
    __shared__ __align__(16) float xs[XS_F];
    const int r = blockIdx.x, tid = threadIdx.x;
    stage_image<true>(depth + (size_t)r * PIXN, xs, img + (size_t)r * PIXN, clip, scale);
    const size_t row = (size_t)r * OBS;
    for (int c = tid; c < (teacher ? OBS : PROP); c += ST) {
        const float e = sanitise(env[row + c]);
        if (teacher) teacher[row + c] = e;
        if (c < PROP) slot[row + c] = e;
    }
    for (int o = tid; o < FEAT; o += ST) {
        const int i = o / FS, j = o - FS * i;
        slot[row + PROP + o] = stem_feature(xs, prm, i, j);   // a plain store: the next act launch reads this slot
    }
    // the record's bookkeeping, rover_dagger_record's, over the grid's n * 512 threads
    const size_t gid = (size_t)r * ST + tid, threads = (size_t)n * ST;
    if (R.rew_out && gid < (size_t)n) {
        R.rew_out[gid] = R.rew[gid];
        R.term_out[gid] = R.terminated[gid] != 0 ? 1 : 0;
    }
    if (R.ring_pos_entry && gid == 0) *R.ring_pos_entry = R.ring_pos_value;
    if (R.idx_out)
        for (size_t g = gid; g < (size_t)R.batch; g += threads) {
            uint32_t w4[4];
            philox4x32((uint32_t)(g >> 2), R.ctr_lo, R.ctr_hi, INDEX_TAG, R.seed_lo, R.seed_hi, w4);
            const uint32_t w = (g & 2) ? ((g & 1) ? w4[3] : w4[2]) : ((g & 1) ? w4[1] : w4[0]);
            R.idx_out[g] = (int64_t)(((uint64_t)w * R.mem_rows) >> 32);   // mem_rows <= 2^32: the product fits 64 bits
        }
}

// ---- update, forward: sampled row r (ring row ro[r] of both rings) into the gathered row r: columns 0 .. 3 from the observation
// ring, the features from the image.  Also what the later kernels of this row need: the identity row number the dense kernels
// index the gathered rows by, and the zero columns of dRow.
__global__ __launch_bounds__(ST) void dagger_conv_forward_kernel(const float *__restrict__ prm, const float *__restrict__ img_ring,
                                                                 const float *__restrict__ obs_ring, const int64_t *__restrict__ ro,
                                                                 float *__restrict__ rows, int64_t *__restrict__ ident,
                                                                 float *__restrict__ drow)
{
    __shared__ __align__(16) float xs[XS_F];
    const int r = blockIdx.x, tid = threadIdx.x;
    const size_t src = (size_t)ro[r], row = (size_t)r * OBS;
    stage_image<false>(img_ring + src * PIXN, xs, nullptr, 0.0f, 0.0f);
    if (tid < PROP) {
        rows[row + tid] = obs_ring[src * OBS + tid];
        drow[row + tid] = 0.0f;
    }
    if (tid == PROP) {
        ident[r] = r;
        drow[row + OBS - 1] = 0.0f;                           // feature (30, 30): the encoder never reads it
    }
    for (int o = tid; o < FEAT; o += ST) {
        const int i = o / FS, j = o - FS * i;
        rows[row + PROP + o] = stem_feature(xs, prm, i, j);
    }
}

// ---- update, backward: workgroup b owns sampled rows [8 b, 8 b + 8).  Wave w owns outputs [128 w, 128 w + 128) of every row as
// two groups of 64, one output per lane: the lane recomputes pre, adds its db2 / dw2 / db1 terms, and hands dpre to its wave
// through LDS in the A-operand order of v_mfma_f32_16x16x4_f32 (i = channel, k = output); the B operand (k = output, j = tap) is
// read from the LDS image, so dW1[c][tap] accumulates over the wave's outputs and the chunk's rows in four 16-tap tiles.  Then
// the waves' tiles are added in wave order and the 17 per-thread sums go through a fixed halving tree; the chunk's 512 floats
// (497 and zeros) go to part[b].
__global__ __launch_bounds__(ST, 4) void dagger_conv_backward_kernel(const float *__restrict__ prm, const float *__restrict__ img_ring,
                                                                  const int64_t *__restrict__ ro, const float *__restrict__ drow,
                                                                  int n, float *__restrict__ part)
{
    __shared__ __align__(16) float xs[XS_F];
    __shared__ float dps[SWAVES][CCH][DPP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rr = lane >> 4, cc = lane & 15;
    const int r0 = blockIdx.x * RC, r1 = min(r0 + RC, n);
    v4f acc[4];
    int toff[4];
    bool tok[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        acc[t] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
        const int tau = 16 * t + cc, u = tau / KW;
        tok[t] = tau < TAPS;
        toff[t] = tok[t] ? u * IW + (tau - KW * u) : 0;
    }
    float sb1[CCH], sw2[CCH], sb2 = 0.0f;
#pragma unroll
    for (int c = 0; c < CCH; ++c) sb1[c] = sw2[c] = 0.0f;
    for (int r = r0; r < r1; ++r) {
        __syncthreads();                                      // the previous row's readers are done with xs
        stage_image<false>(img_ring + (size_t)ro[r] * PIXN, xs, nullptr, 0.0f, 0.0f);
        const float *grow = drow + (size_t)r * OBS + PROP;
#pragma unroll 1
        for (int gi = 0; gi < 2; ++gi) {
            const int g0 = (2 * wave + gi) * 64;
            {
                const int o = g0 + lane;
                const bool ok = o < FEAT;
                const int oc = ok ? o : 0, i = oc / FS, j = oc - FS * i;
                float pre[CCH];
                stem_pre(xs, prm, i, j, pre);
                const float g = ok ? grow[o] : 0.0f;
                sb2 = sb2 + g;
#pragma unroll
                for (int c = 0; c < CCH; ++c) {
                    const float h = leaky(pre[c], 0.01f);
                    sw2[c] = sw2[c] + g * h;
                    const float gw = g * prm[O_W2 + c];
                    const float dp = ok ? (pre[c] > 0.0f ? gw : gw * 0.01f) : 0.0f;
                    sb1[c] = sb1[c] + dp;
                    dps[wave][c][lane] = dp;
                }
            }
            __syncthreads();                                  // dpre of the group is in LDS (every wave runs both groups)
#pragma unroll 2
            for (int s = 0; s < 16; ++s) {
                const int ol = 4 * s + rr, ob = g0 + ol;
                const bool okb = ob < FEAT;
                const int obc = okb ? ob : 0, ib = obc / FS, jb = obc - FS * ib;
                const float *wb = xs + (SH * ib) * IW + SW * jb;
                const float a = cc < CCH ? dps[wave][cc & (CCH - 1)][ol] : 0.0f;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float b = (tok[t] && okb) ? wb[toff[t]] : 0.0f;
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[t], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();                                          // xs becomes the reductions' scratch
    // lane holds D[i = 4 rr + jj][j = cc] of tile t: dW1[c = i][tap = 16 t + j]
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) xs[wave * 1024 + (t * 4 + jj) * 64 + lane] = acc[t][jj];
    __syncthreads();
    float *p = part + (size_t)blockIdx.x * STEM_PAD;
    if (tid < O_B1) {
        const int c = tid / TAPS, tau = tid - TAPS * c;
        const int at = ((tau >> 4) * 4 + (c & 3)) * 64 + (c >> 2) * 16 + (tau & 15);
        float s = xs[at];
        for (int w = 1; w < SWAVES; ++w) s = s + xs[w * 1024 + at];
        p[O_W1 + tid] = s;
    } else if (tid >= STEM_F) {
        p[tid] = 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CCH; ++c) {
        xs[c * ST + tid] = sb1[c];
        xs[(CCH + c) * ST + tid] = sw2[c];
    }
    xs[2 * CCH * ST + tid] = sb2;
    __syncthreads();
    for (int s = ST / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < NSUM; ++k) xs[k * ST + tid] = xs[k * ST + tid] + xs[k * ST + tid + s];
        __syncthreads();
    }
    if (tid < NSUM) p[O_B1 + tid] = xs[tid * ST];             // b1[8], w2[8], b2: the order of the packed stem
}

// ---- host side: the vector is [head | stem], head_floats() + STEM_PAD floats
size_t param_floats() { return head_floats() + STEM_PAD; }

// workspace: dagger_tail.hpp's, with ident (int64 per row) behind ro_n, the gathered rows and dRow (965 floats per row each) in
// front of the network region, and the stem's chunk partials at the end
size_t ws_floats(int rows)
{
    const size_t R = (size_t)rows;
    return ws_shared_floats(rows) + 2 * al4(R) + 2 * al4((size_t)OBS * R) + (size_t)cdiv(rows, RC) * STEM_PAD;
}
struct ConvWs : Ws {
    int64_t *ident;
    float *rows, *drow, *spart;
};
ConvWs ws_at(void *ws, int rows)
{
    ConvWs w = {};
    const size_t R = (size_t)rows;
    float *ident;
    w.spart = ws_carve(w, ws, rows, 2 * al4(R), &ident, 2 * al4((size_t)OBS * R), &w.rows);
    w.ident = reinterpret_cast<int64_t *>(ident);
    w.drow = w.rows + al4((size_t)OBS * R);
    return w;
}

}  // namespace

extern "C" {

size_t rover_dagger_conv_stem_floats(void) { return STEM_F; }
size_t rover_dagger_conv_param_floats(const rover_policy_desc *student)
{
    return is_net(student, false, ROVER_ACT_TANH, true) ? param_floats() : 0;
}
size_t rover_dagger_conv_stem_offset(const rover_policy_desc *student)
{
    return is_net(student, false, ROVER_ACT_TANH, true) ? head_floats() : 0;
}
int32_t rover_dagger_conv_chunk_rows(void) { return RC; }
size_t rover_dagger_conv_workspace_bytes(int32_t max_rows) { return max_rows > 0 ? sizeof(float) * ws_floats(max_rows) : 0; }

int rover_dagger_conv_rows(const rover_dagger_hparams *h, const float *stem, const float *depth, int32_t img_h, int32_t img_w,
                           const float *env_raw, int32_t n, float *ring_slot_out, float *image_slot_out, float *teacher_rows_out,
                           const float *rew, const uint8_t *terminated, float *rew_out, uint8_t *term_out, int32_t *ring_pos_entry,
                           int32_t ring_pos_value, int64_t *idx_out, int32_t batch, int64_t mem_rows, uint64_t counter, void *stream)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "rover_dagger_conv_rows: hparams is NULL");
    if (img_h != IH || img_w != IW)
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "rover_dagger_conv_rows: the stem reads 90 x 160 images only");
    if (!stem || !depth || !env_raw || !ring_slot_out || !image_slot_out)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_dagger_conv_rows: NULL argument");
    if (n < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_dagger_conv_rows: n must be >= 1");
    if (!(h->depth_clip > 0.0f) || !(h->depth_clip < INFINITY) || !(h->depth_scale == h->depth_scale))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_dagger_conv_rows: depth_clip must be positive and finite, depth_scale a number");
    if (misaligned(depth) || misaligned(image_slot_out))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_dagger_conv_rows: depth and image_slot_out must be 16-byte aligned");
    const size_t rb = (size_t)n * OBS * sizeof(float), ib = (size_t)n * PIXN * sizeof(float);
    if (overlap(ring_slot_out, rb, env_raw, rb) || overlap(ring_slot_out, rb, depth, ib) || overlap(image_slot_out, ib, depth, ib) ||
        overlap(image_slot_out, ib, env_raw, rb) || overlap(image_slot_out, ib, ring_slot_out, rb) ||
        overlap(stem, STEM_F * sizeof(float), ring_slot_out, rb) || overlap(stem, STEM_F * sizeof(float), image_slot_out, ib) ||
        (teacher_rows_out && (overlap(teacher_rows_out, rb, env_raw, rb) || overlap(teacher_rows_out, rb, depth, ib) ||
                              overlap(teacher_rows_out, rb, ring_slot_out, rb) || overlap(teacher_rows_out, rb, image_slot_out, ib) ||
                              overlap(teacher_rows_out, rb, stem, STEM_F * sizeof(float)))))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_dagger_conv_rows: the outputs must not alias the inputs or each other");
    if (int rc = rec_check("rover_dagger_conv_rows", rew, terminated, rew_out, term_out, idx_out, batch, mem_rows)) return rc;
    const RecFields R = rec_fill(h, counter, rew, terminated, rew_out, term_out, ring_pos_entry, ring_pos_value, idx_out, batch, mem_rows);
    hipLaunchKernelGGL(rover_dagger_conv_rows_kernel, dim3((unsigned)n), dim3(ST), 0, static_cast<hipStream_t>(stream), stem, depth,
                       env_raw, ring_slot_out, image_slot_out, teacher_rows_out, (int)n, h->depth_clip, h->depth_scale, R);
    return launched("rover_dagger_conv_rows_kernel launch: %s");
}

int rover_dagger_conv_update(const rover_policy_desc *student, const rover_dagger_hparams *h, float *params, float *grad,
                             float *adam_m, float *adam_v, const float *obs_ring, const float *image_ring, int32_t image_slots,
                             int32_t img_h, int32_t img_w, int32_t slots, int32_t num_envs, const int32_t *ring_pos,
                             const float *labels, const int64_t *idx, int32_t n, int64_t valid_rows, void *ws, size_t ws_bytes,
                             void *state, float *replicas, int32_t n_copies, float *dz_out, float *rows_out, float *drow_out,
                             void *stream)
{
    const UpdateImage im = {img_h == IH && img_w == IW, image_ring, image_slots};
    if (int rc = update_check(student, h, params, grad, adam_m, adam_v, obs_ring, slots, num_envs, ring_pos, labels, idx, n, valid_rows,
                              ws, ws_bytes, rover_dagger_conv_workspace_bytes(n), state, replicas, n_copies, &im))
        return rc;
    int dev;
    if (int rc = device_of(params, &dev)) return rc;
    DeviceGuard guard(dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    rover_dagger_state *st = static_cast<rover_dagger_state *>(state);
    ConvWs w = ws_at(ws, n);
    float *rows = rows_out ? rows_out : w.rows, *drow = drow_out ? drow_out : w.drow;
    const int PH = (int)net_floats(false), P = (int)param_floats();
    const size_t so = head_floats();
    const float *stem = params + so;
    const Net pi = net_at(student, params, false);
    if (int rc = gather(w, idx, n, valid_rows, num_envs, slots, ring_pos, nullptr, nullptr, nullptr, st, s)) return rc;
    hipLaunchKernelGGL(dagger_conv_forward_kernel, dim3((unsigned)n), dim3(ST), 0, s, stem, image_ring, obs_ring,
                       (const int64_t *)w.ro_s, rows, w.ident, drow);
    if (int rc = launched("dagger_conv_forward_kernel launch: %s")) return rc;
    FwdJob job = {pi, w.ident, nullptr, 0, &w.reg};
    if (int rc = forward<State>(&job, 1, rows, n, s)) return rc;
    if (int rc = dagger_head(w, labels, idx, valid_rows, n, dz_out, s)) return rc;
    Region *regs[1] = {&w.reg};
    for (int l = NL - 1; l >= 1; --l)
        if (int rc = back_layer<State>(&pi, regs, 1, l, n, s)) return rc;
    {
        // the input gradient: dRow[r][4 + p] = sum_j dZ1[r][j] W1[j][1 + p], p < 960; no activation derivative
        BackLaunch L = {};
        L.rows = n;
        L.slope = 0.01f;
        Back &B = L.d[0];
        B.dz = w.reg.scr[0]; B.dzp = MW[0];
        B.W = pi.p + pi.w_off[0]; B.K = AK[0]; B.N = LN[0];
        B.aref = nullptr; B.arp = 0;
        B.out = drow; B.op = OBS; B.ocol = 1 - PROP;          // column k - ocol = 4 + (k - 1)
        B.k0 = 1; B.nk = FEAT - 1;
        hipLaunchKernelGGL(offpolicy_back_kernel<State>, dim3(cdiv(n, 64), cdiv(B.nk, 64), 1), dim3(FT), 0, s, L);
        if (int rc = launched("offpolicy_back_kernel (input gradient) launch: %s")) return rc;
    }
    const int nch = cdiv(n, RC);
    hipLaunchKernelGGL(dagger_conv_backward_kernel, dim3((unsigned)nch), dim3(ST), 0, s, stem, image_ring, (const int64_t *)w.ro_s,
                       (const float *)drow, (int)n, w.spart);
    if (int rc = launched("dagger_conv_backward_kernel launch: %s")) return rc;
    hipLaunchKernelGGL(offpolicy_combine_kernel<State>, dim3(cdiv(STEM_PAD, FT)), dim3(FT), 0, s, (const float *)w.spart, nch, STEM_PAD,
                       grad + so);
    if (int rc = launched("offpolicy_combine_kernel (stem) launch: %s")) return rc;
    if (int rc = wgrad<State>(&pi, regs, w.ident, 1, rows, n, w.part, grad, s)) return rc;
    return dagger_tail(h, params, grad, adam_m, adam_v, P, PH, w, n, st, replicas, n_copies, s);
}

}  // extern "C"
