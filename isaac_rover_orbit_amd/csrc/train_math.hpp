// train_math.hpp -- the scalar device math the trainers and collectors share (gfx950 / CDNA4): the Cephes expf / tanhf sequences,
// torch's NaN-keeping clamp and min, its nan_to_num of the observation rows, the two activations and Philox4x32-10.
//
// A collector and the update that recomputes its numbers are bit-exact only while both run the same fp32 sequence; they now
// include this one text.  Everything here is force-inlined, so a kernel compiles to what it was with the text in place.
// One restatement remains: policy_kernels.hip (rv_expf, rv_tanhf), rover_kernels.hip and lift_kernels.hip (Philox) keep their
// own copies, because those files' text does not move (they are what bench.py times).  A change here has to be made
// there too, and oracle/policy_oracle.c holds the host-side twin of the two Cephes sequences.
#ifndef ROVER_TRAIN_MATH_HPP
#define ROVER_TRAIN_MATH_HPP

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace {

// Cephes expf / tanhf as explicit fp32 sequences: the same text as policy_kernels.hip and oracle/policy_oracle.c
__device__ __forceinline__ float rv_expf(float x)
{
    if (x > 88.0f) return INFINITY;
    if (x < -88.0f) return 0.0f;
    const float z = floorf(1.44269504088896341f * x + 0.5f);
    x = x - z * 0.693359375f;
    x = x - z * -2.12194440e-4f;
    const float zz = x * x;
    float p = 1.9875691500e-4f;
    p = p * x + 1.3981999507e-3f;
    p = p * x + 8.3334519073e-3f;
    p = p * x + 4.1665795894e-2f;
    p = p * x + 1.6666665459e-1f;
    p = p * x + 5.0000001201e-1f;
    p = p * zz + x + 1.0f;
    return ldexpf(p, (int)z);
}
__device__ __forceinline__ float rv_tanhf(float x)
{
    const float z = fabsf(x);
    if (z > 44.0f) return x > 0.0f ? 1.0f : -1.0f;
    if (z >= 0.625f) {
        const float s = rv_expf(z + z);
        const float r = 1.0f - 2.0f / (s + 1.0f);
        return x < 0.0f ? -r : r;
    }
    if (x == 0.0f) return x;
    const float s = x * x;
    float p = -5.70498872745e-3f;
    p = p * s + 2.06390887954e-2f;
    p = p * s - 5.37397155531e-2f;
    p = p * s + 1.33314422036e-1f;
    p = p * s - 3.33332819422e-1f;
    return p * s * x + x;
}

// torch.clamp: a NaN stays a NaN
__device__ __forceinline__ float tclamp(float x, float lo, float hi) { return x != x ? x : fminf(fmaxf(x, lo), hi); }
// torch.min: NaN if either is NaN
__device__ __forceinline__ float tmin(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (a < b ? a : b); }

// torch.nan_to_num(x, nan = 0, posinf = FLT_MAX, neginf = 0): finite values (and -0) pass unchanged
__device__ __forceinline__ float sanitise(float x)
{
    if (x != x) return 0.0f;
    if (x == INFINITY) return FLT_MAX;
    if (x == -INFINITY) return 0.0f;
    return x;
}

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.0f ? v : v * slope; }
// ELU exactly as policy_kernels.hip's activate(): rover_policy.h fixes expm1f
__device__ __forceinline__ float elu(float v) { return v > 0.0f ? v : expm1f(v); }

// Philox4x32-10 (the text of rover_kernels.hip)
__device__ __forceinline__ void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// a Philox word as a uniform inside (0, 1): ((w >> 9) + 0.5) * 2^-23, exact in fp32
__device__ __forceinline__ float unit_uniform(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 0x1p-23f; }
// the standard normal pair of two Philox words (the Box-Muller form and sincospif of rover_rollout.h): the angle 2 pi u2 with an
// exact argument, e0 on the cosine and e1 on the sine
__device__ __forceinline__ void box_muller(uint32_t w0, uint32_t w1, float &e0, float &e1)
{
    const float u1 = unit_uniform(w0), u2 = unit_uniform(w1);
    const float rho = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    e0 = rho * cs;
    e1 = rho * sn;
}

}  // namespace

#endif  // ROVER_TRAIN_MATH_HPP
