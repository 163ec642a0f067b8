// lift_rollout_kernels.hip -- the on-policy rollout step of the lift task in one launch (gfx950 / CDNA4, wave64): copy the env's raw
// observation rows into the rollout buffer, standardise them with the state scaler, run the actor and the critic, undo the value
// scaler, draw counter-based Gaussian actions and evaluate the log-probability.  See include/rover_lift_rollout.h for the contract.
//
// The network part is the forward half of lift_rows_kernel (lift_ppo_kernels.hip), which restates rover_policy_forward's generic
// kernel: per 16 x 16 output tile the same v_mfma_f32_16x16x4_f32 sequence (k groups ascending, the ragged k >= 36 lanes fed as
// zeros), the same bias add, the same ELU, so mean and value are bit-identical to FusedLiftPPO.actor / .critic on
// FusedLiftPPO.standardize(rows), and to what the update recomputes (tests/test_gpu_lift_rollout.py pins the three together).
// The text is restated here and not shared: lift_ppo_kernels.hip, policy_kernels.hip and rollout_kernels.hip stay byte for byte
// what they were, so their registers, schedules and times cannot move.  The sampling epilogue is rover_rollout_act_kernel's
// (the same Philox / Box-Muller device sequence under a tag of its own), on the lanes that hold the actor's final MFMA sums:
// lane (column c = lane & 15, quad q = lane >> 4) owns rows 4 q .. 4 q + 3 of column c, nothing passes through LDS.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rover_hip.h"
#include "../../include/rover_lift_rollout.h"
#include "../../include/rover_policy.h"
#include "rover_internal.hpp"
#include "train_math.hpp"
#include "train_shared.hpp"   // cdiv, the packed sizes

namespace {

constexpr int OBS = 36;
constexpr int NL = 4;
constexpr int LK[NL] = {36, 256, 128, 64};           // in features of the lift layers
constexpr int LN[NL - 1] = {256, 128, 64};           // out features of layers 1 .. 3 (layer 4: A actor, 1 critic)
constexpr int RB = 16;                               // rows per workgroup = M of the MFMA tile
constexpr int RT = 512;                              // threads (8 waves)
constexpr int MAX_ACT = 16;                          // one column tile
// LDS pitches of the row buffers (columns + 4), as lift_rows_kernel
constexpr int PX = 40, P1 = 260, P2 = 132, P3 = 68;
constexpr int NET_F = RB * (P1 + P2 + P3);
constexpr int LDS_FLOATS = RB * PX + 2 * NET_F;      // 15360 floats = 61440 bytes
constexpr uint32_t LRO_TAG = 0x4C524F00u;            // "LRO\0": word 3 of the Philox counter, | action pair

__device__ __forceinline__ float clampf_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }   // NaN passes
// RunningStandardScaler forward / inverse (rover_lift_train.h), fp32 with explicit roundings: the text of lift_ppo_kernels.hip
__device__ __forceinline__ float scaler_fwd(float x, double mean, double var, float eps, float clip)
{
    const float d = __fadd_rn(sqrtf((float)var), eps);
    return clampf_nan(__fdiv_rn(__fsub_rn(x, (float)mean), d), -clip, clip);
}
__device__ __forceinline__ float scaler_inv(float x, double mean, double var, float clip)
{
    return __fadd_rn(__fmul_rn(sqrtf((float)var), clampf_nan(x, -clip, clip)), (float)mean);
}

// one 16 x 16 output tile of a forward layer: rover_policy_forward's MFMA sequence (k groups ascending, k = 16 g + 4 j + akq)
template <int K>
__device__ __forceinline__ v4f fwd_tile(const float *in, int ip, const v4f *Wt, int arow, int akq)
{
    constexpr int G = (K + 15) / 16;
    v4f b[G];
#pragma unroll
    for (int g = 0; g < G; ++g) b[g] = Wt[(size_t)g * 64];
    __builtin_amdgcn_sched_barrier(0);   // every B fragment of the tile is in flight before the first MFMA waits for one
    v4f acc = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    const float *ap = in + arow * ip + akq;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 16 * g + 4 * j + akq;
            const float a = (K % 16 == 0 || k < K) ? ap[16 * g + 4 * j] : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[g][j], acc, 0, 0, 0);
        }
    return acc;
}

struct LroArgs {
    uint32_t w_off[2][NL], b_off[2][NL];   // actor / critic layer offsets inside one packed replica
    unsigned copy_floats[2];               // floats of one replica
    int n_copies;                          // workgroup b reads replica b % n_copies
    int nout;                              // A
    rover_lift_rollout_hparams hp;
    uint32_t ctr_lo, ctr_hi;
    const float *obs, *log_std;
    const double *state_scaler, *value_scaler;
    int n;
    float *obs_out, *mean_out, *val_out, *act_out, *env_act_out, *logp_out, *eps_out;
};

__global__ __launch_bounds__(RT) void lift_rollout_act_kernel(LroArgs A, const float *__restrict__ packed_a,
                                                              const float *__restrict__ packed_b)
{
    __shared__ __align__(16) float lds[LDS_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int arow = lane & 15, akq = lane >> 4;
    const int row0 = blockIdx.x * RB, rows = min(RB, A.n - row0);
    const unsigned copy = blockIdx.x % (unsigned)A.n_copies;
    packed_a += (size_t)copy * A.copy_floats[0];
    packed_b += (size_t)copy * A.copy_floats[1];
    float *X = lds;
    auto y1 = [&](int net) __attribute__((always_inline)) { return lds + RB * PX + net * NET_F; };
    auto y2 = [&](int net) __attribute__((always_inline)) { return y1(net) + RB * P1; };
    auto y3 = [&](int net) __attribute__((always_inline)) { return y2(net) + RB * P2; };
    auto Wl = [&](int net, int l) __attribute__((always_inline)) { return (net ? packed_b : packed_a) + A.w_off[net][l]; };
    auto Bl = [&](int net, int l) __attribute__((always_inline)) { return (net ? packed_b : packed_a) + A.b_off[net][l]; };

    // ---- raw rows -> the rollout buffer (unchanged) and, standardised by the state scaler, the LDS tile; rows past n are zeros
    for (int e = tid; e < RB * OBS; e += RT) {
        const int r = e / OBS, c = e - r * OBS;
        float v = 0.0f;
        if (r < rows) {
            const float o = A.obs[(size_t)row0 * OBS + e];
            if (A.obs_out) A.obs_out[(size_t)row0 * OBS + e] = o;
            v = scaler_fwd(o, A.state_scaler[c], A.state_scaler[OBS + c], A.hp.scaler_eps, A.hp.scaler_clip);
        }
        X[r * PX + c] = v;
    }
    __syncthreads();

    // ---- hidden layers, both networks: wave-uniform loop over (network, column tile) items
    auto layer = [&](auto k_tag, int l, auto in_of, int ip, auto out_of, int op) __attribute__((always_inline)) {
        constexpr int K = decltype(k_tag)::value;
        const int T = LN[l] / 16;
        for (int tt = wave; tt < 2 * T; tt += RT / 64) {
            const int net = tt / T, t = tt - net * T;
            const v4f *Wt = reinterpret_cast<const v4f *>(Wl(net, l)) + (size_t)t * ((K + 15) / 16) * 64 + lane;
            const float bv = Bl(net, l)[16 * t + arow];
            const v4f acc = fwd_tile<K>(in_of(net), ip, Wt, arow, akq);
            float *dst = out_of(net) + 16 * t + arow;
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[(4 * akq + j) * op] = elu(acc[j] + bv);
        }
        __syncthreads();
    };
    auto xin = [&](int) __attribute__((always_inline)) { return (const float *)X; };
    layer(std::integral_constant<int, 36>{}, 0, xin, PX, y1, P1);
    layer(std::integral_constant<int, 256>{}, 1, y1, P1, y2, P2);
    layer(std::integral_constant<int, 128>{}, 2, y2, P2, y3, P3);

    // ---- output layer: wave 0 the actor's one column tile, wave 1 the critic's; the sums stay in the lanes that hold them
    if (wave >= 2) return;
    const int net = wave;
    const int N = net ? 1 : A.nout;
    const int c = arow;                                                 // the lane's output column
    const float bv = Bl(net, 3)[min(c, N - 1)];
    const v4f acc = fwd_tile<64>(y3(net), P3, reinterpret_cast<const v4f *>(Wl(net, 3)) + lane, arow, akq);
    if (net) {   // the value leaves from the lane that holds it
        if (c == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = 4 * akq + j;
                const float v = acc[j] + bv;
                if (r < rows)
                    A.val_out[row0 + r] = A.value_scaler ? scaler_inv(v, A.value_scaler[0], A.value_scaler[1], A.hp.scaler_clip) : v;
            }
        }
        return;
    }
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        y[j] = acc[j] + bv;                                             // the policy mean (no final activation)
        if (4 * akq + j < rows && c < N) A.mean_out[(size_t)(row0 + 4 * akq + j) * N + c] = y[j];
    }

    // ---- sampling epilogue (rover_rollout_act_kernel's, per owned row): lane (q, c) owns action column c of rows 4 q .. 4 q + 3
    const bool draw = A.act_out || A.env_act_out || A.logp_out || A.eps_out;
    if (!draw) return;
    const float ls = fminf(fmaxf(A.log_std[min(c, N - 1)], A.hp.log_std_min), A.hp.log_std_max);
    const float sd = expf(ls);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = 4 * akq + j;
        uint32_t w4[4];
        philox4x32((uint32_t)A.hp.env_id_offset + (uint32_t)(row0 + r), A.ctr_lo, A.ctr_hi, LRO_TAG | (uint32_t)(c >> 1), A.hp.seed_lo, A.hp.seed_hi, w4);
        const float u1 = ((float)(w4[0] >> 9) + 0.5f) * 0x1p-23f, u2 = ((float)(w4[1] >> 9) + 0.5f) * 0x1p-23f;   // exact, inside (0, 1)
        const float rho = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincospif(2.0f * u2, &sn, &cs);         // the angle 2 pi u2 with an exact argument
        const float eps = (c & 1) ? rho * sn : rho * cs;
        const float noise = sd * eps;
        const float a = y[j] + noise;           // a separate multiply and add
        const float cl = fminf(fmaxf(a, A.hp.action_low), A.hp.action_high);
        const float ea = (A.hp.clip_actions && a == a) ? cl : a;   // torch.clamp keeps a NaN; fmaxf alone would turn it into action_low
        const float x = (a - y[j]) / sd;        // lift_rows_kernel forms x, the term and the row sum below the same way
        const float term = -0.5f * x * x - ls - 0.9189385332f;
        float lp = 0.0f;                        // column 0 first, then the others in order (all 64 lanes take part)
        for (int k = 0; k < N; ++k) lp = lp + __shfl(term, (lane & ~15) + k);
        const size_t o = (size_t)(row0 + r) * N + c;
        if (r < rows && c < N) {
            if (A.eps_out) A.eps_out[o] = eps;
            if (A.act_out) A.act_out[o] = a;
            if (A.env_act_out) A.env_act_out[o] = ea;
        }
        if (A.logp_out && c == 0 && r < rows) A.logp_out[row0 + r] = lp;
    }
}

__global__ __launch_bounds__(256) void lift_rollout_record_kernel(const float *__restrict__ rew, const uint8_t *__restrict__ terminated,
                                                                  const uint8_t *__restrict__ truncated, int n, float reward_scale,
                                                                  const float *__restrict__ log, float *__restrict__ rew_out,
                                                                  float *__restrict__ done_out, float *__restrict__ ep_sum,
                                                                  float *__restrict__ ep_count)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        rew_out[i] = rew[i] * reward_scale;
        done_out[i] = (terminated[i] | truncated[i]) ? 1.0f : 0.0f;
    }
    if (i == 0 && log) {   // one thread: the envs reset in this step (log[0:8] are their means / counts, log[8] their number)
        const float k = log[8];
        if (k > 0.0f) {
#pragma unroll
            for (int j = 0; j < 8; ++j) ep_sum[j] = ep_sum[j] + log[j] * (j < 6 ? k : 1.0f);
            ep_count[0] = ep_count[0] + k;
        }
    }
}

// rover_lift_policy_desc(nout) with the offsets rover_policy_pack sets
bool is_lift(const rover_policy_desc *d, int nout)
{
    if (d->obs_dim != OBS || d->prop_dim != OBS || d->n_enc != 0 || d->n_mlp != NL) return false;
    size_t off = 0;
    for (int i = 0; i < NL; ++i) {
        const rover_policy_layer &l = d->layers[i];
        if (l.K != LK[i] || l.N != (i < NL - 1 ? LN[i] : nout)) return false;
        if (l.act != (i < NL - 1 ? ROVER_ACT_ELU : ROVER_ACT_NONE) || l.split_k != 0) return false;
        if (l.w_off != off) return false;
        off += layer_weight_floats(l);
        if (l.b_off != off) return false;
        off += layer_bias_floats(l);
    }
    return true;
}

}  // namespace

extern "C" {

int rover_lift_rollout_default_hparams(rover_lift_rollout_hparams *h)
{
    if (!h) return rover_internal_fail(ROVER_ERR_INVALID, "hparams is NULL");
    memset(h, 0, sizeof(*h));
    h->seed_lo = 42u; h->seed_hi = 0u;
    h->env_id_offset = 0;
    h->clip_actions = 0;                              // skrl_ppo_cfg.yaml: clip_actions: False
    h->action_low = -1.0f; h->action_high = 1.0f;
    h->log_std_min = -20.0f; h->log_std_max = 2.0f;
    h->scaler_eps = 1e-8f; h->scaler_clip = 5.0f;
    h->reward_scale = 0.01f;
    return ROVER_OK;
}

size_t rover_lift_rollout_hparams_bytes(void) { return sizeof(rover_lift_rollout_hparams); }

int rover_lift_rollout_act(const rover_policy_desc *actor, const float *packed_a, const rover_policy_desc *critic, const float *packed_b,
                           int32_t n_copies, const rover_lift_rollout_hparams *h, uint64_t counter, const float *obs, int32_t n,
                           const float *log_std, const double *state_scaler, const double *value_scaler, float *obs_out,
                           float *mean_out, float *val_out, float *act_out, float *env_act_out, float *logp_out, float *eps_out,
                           void *stream)
{
    if (!actor || !critic || !h) return rover_internal_fail(ROVER_ERR_INVALID, "rover_lift_rollout_act: NULL descriptor / hparams");
    if (!packed_a || !packed_b || !obs || !log_std || !state_scaler || !mean_out || !val_out)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_lift_rollout_act: NULL required pointer");
    if (n < 1 || n_copies < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_lift_rollout_act: n and n_copies must be >= 1");
    if ((reinterpret_cast<uintptr_t>(packed_a) | reinterpret_cast<uintptr_t>(packed_b)) & 15)
        return rover_internal_fail(ROVER_ERR_INVALID, "packed weights must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(state_scaler) | reinterpret_cast<uintptr_t>(value_scaler)) & 7)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_lift_rollout_act: scaler blocks must be 8-byte aligned");
    if (!(h->log_std_min <= h->log_std_max)) return rover_internal_fail(ROVER_ERR_INVALID, "rover_lift_rollout_act: log_std_min > log_std_max");
    if (h->clip_actions && !(h->action_low <= h->action_high))
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_lift_rollout_act: action_low > action_high");
    if (!(h->scaler_clip >= 0.0f)) return rover_internal_fail(ROVER_ERR_INVALID, "rover_lift_rollout_act: scaler_clip must be >= 0");
    if (obs_out == obs) return rover_internal_fail(ROVER_ERR_INVALID, "rover_lift_rollout_act: obs_out must not alias obs");
    const int A = actor->layers[NL - 1].N;
    if (A < 1 || A > MAX_ACT || !is_lift(actor, A) || !is_lift(critic, 1))
        return rover_internal_fail(ROVER_ERR_UNSUPPORTED, "rover_lift_rollout_act: the networks must be rover_lift_policy_desc(A <= 16) and "
                                                          "(1), packed by rover_policy_pack");
    LroArgs L;
    const rover_policy_desc *d[2] = {actor, critic};
    for (int k = 0; k < 2; ++k) {
        for (int i = 0; i < NL; ++i) { L.w_off[k][i] = d[k]->layers[i].w_off; L.b_off[k][i] = d[k]->layers[i].b_off; }
        L.copy_floats[k] = (unsigned)rover_policy_packed_floats(d[k]);
    }
    L.n_copies = n_copies;
    L.nout = A;
    L.hp = *h;
    L.ctr_lo = (uint32_t)(counter & 0xFFFFFFFFu);
    L.ctr_hi = (uint32_t)(counter >> 32);
    L.obs = obs; L.log_std = log_std;
    L.state_scaler = state_scaler; L.value_scaler = value_scaler;
    L.n = n;
    L.obs_out = obs_out; L.mean_out = mean_out; L.val_out = val_out;
    L.act_out = act_out; L.env_act_out = env_act_out; L.logp_out = logp_out; L.eps_out = eps_out;
    hipLaunchKernelGGL(lift_rollout_act_kernel, dim3(cdiv(n, RB)), dim3(RT), 0, static_cast<hipStream_t>(stream), L, packed_a,
                       packed_b);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "lift_rollout_act_kernel launch: %s", hipGetErrorString(e));
    return ROVER_OK;
}

int rover_lift_rollout_record(const float *rew, const uint8_t *terminated, const uint8_t *truncated, int32_t n, float reward_scale,
                              const float *log, float *rew_out, float *done_out, float *ep_sum, float *ep_count, void *stream)
{
    if (!rew || !terminated || !truncated || !rew_out || !done_out)
        return rover_internal_fail(ROVER_ERR_INVALID, "rover_lift_rollout_record: NULL pointer");
    if (log && (!ep_sum || !ep_count)) return rover_internal_fail(ROVER_ERR_INVALID, "rover_lift_rollout_record: log without ep_sum / ep_count");
    if (n < 1) return rover_internal_fail(ROVER_ERR_INVALID, "rover_lift_rollout_record: n must be >= 1");
    hipLaunchKernelGGL(lift_rollout_record_kernel, dim3(cdiv(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), rew, terminated,
                       truncated, (int)n, reward_scale, log, rew_out, done_out, ep_sum, ep_count);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rover_internal_fail(ROVER_ERR_HIP, "lift_rollout_record_kernel launch: %s", hipGetErrorString(e));
    return ROVER_OK;
}

}  // extern "C"
