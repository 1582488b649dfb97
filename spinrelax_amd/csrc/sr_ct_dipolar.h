// sr_ct_dipolar.h -- the scalar (w) series of the distance-weighted correlation kernels: k_ct_dipolar (sr_ct_dipolar.hip: one series
// against itself) and k_ct_dipolar_cross (sr_ct_dipolar_cross.hip: the series of two vectors against each other) stage it in the same
// LDS layout behind the three a planes of sr_ct_shift.h and run the same inner loop on it; k_ct_modes (sr_ct_modes.hip) stages its five
// signal series so and runs the loop on pairs of them.  Also the tile of the two normalising kernels (dip_scale_tile).
//
// A staged w series: Fp = ct_Fp(F) frames, zero behind frame F, parity-split 16-byte chunks, so that the 16 lag-lanes of a
// ds_read_b128 group read 256 consecutive bytes; Hw = Fp / 2 floats per half.
#pragma once
#include "sr_ct_shift.h"

namespace {

// float index of frame e of the w series: 16-byte chunk c (4 frames) lives in half (c & 1) at slot (c >> 1); Hw = Fp / 2 floats per half
__device__ __forceinline__ int lds_wpos(int e, int Hw)
{
    const int c = e >> 2;
    return (c & 1) * Hw + (c >> 1) * 4 + (e & 3);
}

// ct_shift_block for the scalar series: one wave, the block of kLagBlock lags that starts at lag dw, of the staged series lwa (the
// earlier frame) and lwb (the later one); lane (strip g, lag-lane l16) ADDS to acc64[d] its strip's part of sum_j wa(j) wb(j + lag),
// lag = dw + kLagsPerLane l16 + d.  The same strips, the same window rotation (one new 8-frame half per step: 2 + 2 ds_read_b128 per
// 64 FMAs), float32 partial sums of at most 16 terms in [0, 1] started at -center, folded into float64 every kFlush steps.
__device__ __forceinline__ void dip_shift_block_w(const float *lwa, const float *lwb, int Hw, int F, int dw, int g, int l16,
                                                  double (&acc64)[kLagsPerLane], const float center)
{
    const int nj = F - dw;
    const int S = (((nj + 3) >> 2) + 15) & ~15;
    const int iters = S >> 3;
    const float *pa0 = lwa + ((g * S) >> 3) * 4;
    const float *pa1 = pa0 + Hw;
    const float *pb0 = lwb + ((g * S + dw + kLagsPerLane * l16) >> 3) * 4;
    const float *pb1 = pb0 + Hw;
    float P[8], Q[8];
#define SR_DIP_LOAD_HALF(H, OFF)                                                                 \
    {                                                                                        \
        const float4 t0 = *reinterpret_cast<const float4 *>(pb0 + (OFF));                   \
        const float4 u0 = *reinterpret_cast<const float4 *>(pb1 + (OFF));                   \
        H[0] = t0.x; H[1] = t0.y; H[2] = t0.z; H[3] = t0.w; H[4] = u0.x; H[5] = u0.y; H[6] = u0.z; H[7] = u0.w; \
    }
#define SR_DIP_STEP(LO, HI)                                                                      \
    {                                                                                        \
        float a[kJT], b[16];                                                                 \
        {                                                                                    \
            const float4 t = *reinterpret_cast<const float4 *>(pa0);                        \
            const float4 u = *reinterpret_cast<const float4 *>(pa1);                        \
            a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w; a[4] = u.x; a[5] = u.y; a[6] = u.z; a[7] = u.w; \
        }                                                                                    \
        SR_DIP_LOAD_HALF(HI, 4)                                                              \
        _Pragma("unroll") for (int t = 0; t < 8; ++t) { b[t] = LO[t]; b[8 + t] = HI[t]; }    \
        _Pragma("unroll") for (int jj = 0; jj < kJT; ++jj) {                                 \
            _Pragma("unroll") for (int d = 0; d < kLagsPerLane; ++d)                         \
                acc[d][jj & 3] = fmaf(a[jj], b[jj + d], acc[d][jj & 3]);                     \
        }                                                                                    \
        pa0 += 4; pa1 += 4; pb0 += 4; pb1 += 4;                                              \
    }
    SR_DIP_LOAD_HALF(P, 0)
    for (int it0 = 0; it0 < iters; it0 += kFlush) {
        float acc[kLagsPerLane][4];
#pragma unroll
        for (int d = 0; d < kLagsPerLane; ++d)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[d][q] = -center;
        const int n = min(kFlush, iters - it0);            // even
        for (int ii = 0; ii < n; ii += 2) {
            SR_DIP_STEP(P, Q)
            SR_DIP_STEP(Q, P)
        }
#pragma unroll
        for (int d = 0; d < kLagsPerLane; ++d) {
            const float s = (acc[d][0] + acc[d][1]) + (acc[d][2] + acc[d][3]);
            acc64[d] += (double)s + 4.0 * (double)center;
        }
    }
#undef SR_DIP_STEP
#undef SR_DIP_LOAD_HALF
}

// the tile of the two normalising kernels (k_ct_dipolar_norm, k_ct_dipolar_cross_norm), 256 threads: Ct, dCt (L, n) scaled in place,
// the 64 rows from row0 (vectors or pairs) x the 64 lags of blockIdx.x, row row0 + i by inv[i]
__device__ __forceinline__ void dip_scale_tile(const double *inv, int L, int64_t n, int64_t row0, double *Ct, double *dCt)
{
    const int tid = threadIdx.x;
    const int vl = tid & 63;
    const int64_t v = row0 + vl;
    if (v >= n) return;
    for (int i = tid >> 6; i < 64; i += 4) {
        const int d = blockIdx.x * 64 + i;              // lag index - 1
        if (d >= L) break;
        const int64_t o = (int64_t)d * n + v;
        Ct[o] *= inv[vl];
        dCt[o] *= inv[vl];
    }
}

}  // namespace
