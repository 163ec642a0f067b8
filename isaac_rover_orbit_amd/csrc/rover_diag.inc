// Diagnostic builds only (tools/build_diag.py: -DRV_K1_STAMP, -DRV_K1_LITE [-DRV_K1_LITE_FINE]): s_memtime stamps of the step
// kernels' phases.  The product build never includes this file: there K1_STAMP / K1_LITE expand to nothing (rover_kernels.hip).
// Included inside rover_kernels.hip's anonymous namespace.
#pragma once
#if defined(RV_K1_STAMP) || defined(RV_K1_LITE)
__device__ unsigned long long *g_k1_stamps;
#endif
// RV_K1_LITE: a timeline of the one-launch kernel's two waves on SIMD 0 (step wave 0: slots 0.., copy wave 4: slots 16..) from
// stamps that do not wait for anything -- the waiting stamps below serialise the very overlap this timeline is about
#ifdef RV_K1_LITE
__device__ __forceinline__ void k1_lite(int slot)
{
    if ((threadIdx.x & 255) == 0) {
        unsigned long long t;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
        g_k1_stamps[(size_t)blockIdx.x * 64 + (threadIdx.x >> 8) * 32 + slot] = t;
    }
}
#define K1_LITE(k) k1_lite(k)
#endif
#ifdef RV_K1_LITE_FINE   // more stamps inside the manager tail / the first staging (each costs the wave several hundred cycles)
#define K1_LITE_F(k) k1_lite(k)
#endif
#ifdef RV_K1_STAMP
__device__ __forceinline__ void k1_stamp(int slot)
{
    if (threadIdx.x == 0) {
        unsigned long long t;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
        g_k1_stamps[(size_t)blockIdx.x * 32 + slot] = t;
    }
}
#define K1_STAMP(k) k1_stamp(k)
#endif
