// sr_fft_common.h -- what the in-LDS transforms of kernel 1 share whatever their scalar type: the float64 kernels of
// sr_ct_fft64.hip and the float32 ones of sr_ct32_fft.h (k_ct_rfft32, the blocked form).  Index maps, the padded size of a
// transform image, and the DPP wave scans.  The butterflies and the complex arithmetic are NOT here: the float32 ones are
// hand-packed v_pk_* code with special cases of their own (sr_ct32_fft.h), the float64 ones plain fma code (sr_ct_fft64.hip).
#pragma once
#include "sr_internal.h"

namespace {

template <int LOGN>
__host__ __device__ constexpr int bitrev(int p)
{
    int r = 0;
    for (int b = 0; b < LOGN; ++b) r |= ((p >> b) & 1) << (LOGN - 1 - b);
    return r;
}

// Step 1 of a workgroup transform is an in-register transform of a thread's N1 points that leaves X[k1(p)] in v[p].
// N1 a power of two (radix-2 decimation in frequency): bit reversal.  N1 = 12 = 3 x 4 (n1 = 4 a + b, k1 = ka + 3 kb).
template <int N1>
struct Stage1Map {                                         // N1 = 4, 8, 16, 32
    static_assert((N1 & (N1 - 1)) == 0, "a power of two, or a specialisation");
    static constexpr int LOG = N1 == 4 ? 2 : (N1 == 8 ? 3 : (N1 == 16 ? 4 : 5));
    __host__ __device__ static constexpr int k1(int p) { return bitrev<LOG>(p); }
};
template <>
struct Stage1Map<12> {
    __host__ __device__ static constexpr int k1(int p) { return (p >> 2) + 3 * bitrev<2>(p & 3); }
};

// Slots of the LDS image of a real-input transform of half length H = 256 N1: the H points in natural order with one pad slot
// per N1 (256 of them), and 16 behind for the row layout of steps 2 and 3 (rows of 17)
__host__ __device__ constexpr int rfft_img_slots(int N1) { return 256 * N1 + 256 + 16; }

// Hide the thread index's provenance from the optimiser: every LDS / global address of a transform kernel is a function of it,
// and the ~80 addresses of one transform would otherwise be computed once per kernel and spilled.
__device__ __forceinline__ int opaque(int t)
{
    asm volatile("" : "+v"(t));
    return t;
}

// ---- wave scans with DPP moves: row_shr 1, 2, 4, 8 inside the rows of 16 lanes, then row_bcast15 / row_bcast31 (the AMDGPU
// atomic optimiser's sequence); lanes without a source combine with 0.  All inclusive: lane 63 ends up with the wave's result.
#define SR_DPP_SCAN(STEP) STEP(0x111, 0xF) STEP(0x112, 0xF) STEP(0x114, 0xF) STEP(0x118, 0xF) STEP(0x142, 0xA) STEP(0x143, 0xC)
#define SR_DPP_F32(V, CTRL, RM) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, V), CTRL, RM, 0xF, false))
__device__ __forceinline__ float wave_scan_f32(float v)      // inclusive prefix sums
{
#define SR_STEP(CTRL, RM) v += SR_DPP_F32(v, CTRL, RM);
    SR_DPP_SCAN(SR_STEP)
#undef SR_STEP
    return v;
}
__device__ __forceinline__ float wave_total_f32(float v) { return wave_scan_f32(v); }       // for callers that read lane 63 only
__device__ __forceinline__ float wave_max_f32(float v)       // v >= 0: 0 is neutral
{
#define SR_STEP(CTRL, RM) v = fmaxf(v, SR_DPP_F32(v, CTRL, RM));
    SR_DPP_SCAN(SR_STEP)
#undef SR_STEP
    return v;
}
__device__ __forceinline__ double wave_scan_f64(double v)    // inclusive prefix sums
{
    union U { double d; int i[2]; };
#define SR_STEP(CTRL, RM)                                                                        \
    {                                                                                            \
        U a_, b_;                                                                                \
        a_.d = v;                                                                                \
        b_.i[0] = __builtin_amdgcn_update_dpp(0, a_.i[0], CTRL, RM, 0xF, false);                 \
        b_.i[1] = __builtin_amdgcn_update_dpp(0, a_.i[1], CTRL, RM, 0xF, false);                 \
        v += b_.d;                                                                               \
    }
    SR_DPP_SCAN(SR_STEP)
#undef SR_STEP
    return v;
}
#undef SR_DPP_F32
#undef SR_DPP_SCAN

}  // namespace
