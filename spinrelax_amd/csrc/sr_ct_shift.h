// sr_ct_shift.h -- the shifted-product lag block of the staged correlation kernels on xyz series: k_ct_palmer (sr_ct_direct.hip: one
// series against itself), k_ct_cross (sr_ct_cross.hip: two series against each other), k_ct_dipolar (sr_ct_dipolar.hip: the a planes
// against themselves) and k_ct_dipolar_cross (sr_ct_dipolar_cross.hip: the a planes of two vectors) stage their series in the same LDS
// layout and run the same inner loop; the lane map and ct_combine_strips also serve the scalar series of sr_ct_dipolar.h, which
// k_ct_modes (sr_ct_modes.hip) uses alone.  What the five kernels share around the inner loop: sr_ct_staged.h.
//
// A staged series: Fp = ct_Fp(F) frames, zero behind frame F, "chunk-parity split, xyz-interleaved": 16-byte
// chunk c (4 frames of one component) lives in half (c & 1) at slot (c >> 1); a slot is 48 bytes = [x-chunk | y-chunk | z-chunk];
// Hf = (Fp >> 3) * 12 floats per half, 2 Hf = 3 Fp floats per series.  Why this layout, and the lane map below: sr_ct_direct.hip.
#pragma once
#include "sr_internal.h"

namespace {

constexpr int kLagsPerLane = 8;
constexpr int kJT = 8;             // j values per lane step
constexpr int kFlush = 8;          // lane steps between float32 -> float64 folds
constexpr float kCenter = 8.0f;    // accumulators start at -kCenter so the <=16 terms (each in [0,1]) keep
                                   // the running float32 sum near zero: halves the accumulation rounding
constexpr int kPad = 192;          // zero padding behind the series (max overshoot of a window: 190)

__host__ __device__ inline int64_t ct_Fp(int64_t F)
{
    // smallest Fp >= F + kPad with Fp % 64 == 32 (so the two parity halves are 16 banks apart)
    int64_t x = F + kPad;
    int64_t base = (x / 64) * 64 + 32;
    if (base < x) base += 64;
    return base;
}

// float index of frame e, component comp in the interleaved parity-split layout; Hf = floats per half
__device__ __forceinline__ int lds_pos(int e, int comp, int Hf)
{
    const int c = e >> 2;
    return (c & 1) * Hf + (c >> 1) * 12 + comp * 4 + (e & 3);
}

// lane -> (strip g, lag-lane l16) following the ds_read_b128 lane groups, and back
__device__ __forceinline__ void lane_to_strip(int lane, int &g, int &l16)
{
    const int h = lane >> 5, m = lane & 31;
    const bool inA = (m < 4) || (m >= 12 && m < 16) || (m >= 20 && m < 28);
    g = 2 * h + (inA ? 0 : 1);
    if (inA) l16 = m < 4 ? m : (m < 16 ? m - 8 : m - 12);
    else l16 = m < 12 ? m - 4 : (m < 20 ? m - 8 : m - 16);
}
__device__ __forceinline__ int strip_to_lane(int g, int l16)
{
    const int h = g >> 1;
    int m;
    if ((g & 1) == 0) m = l16 < 4 ? l16 : (l16 < 8 ? l16 + 8 : l16 + 12);
    else m = l16 < 8 ? l16 + 4 : (l16 < 12 ? l16 + 8 : l16 + 16);
    return 32 * h + m;
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// stage frames [0, F) of the three planes px, py, pz into the series at s (zero padding up to Fp); coalesced dword loads
template <int NT>
__device__ __forceinline__ void ct_stage_series(float *s, const float *px, const float *py, const float *pz, int F, int Fp, int Hf, int tid)
{
    for (int e = tid; e < Fp; e += NT) {
        const int p = lds_pos(e, 0, Hf);
        const bool in = e < F;
        s[p] = in ? px[e] : 0.f;
        s[p + 4] = in ? py[e] : 0.f;
        s[p + 8] = in ? pz[e] : 0.f;
    }
}

// One wave, the block of kLagBlock lags that starts at lag dw, of the staged series la (the earlier frame) and lb (the later one):
// lane (strip g, lag-lane l16) ADDS to acc64[d] its strip's part of sum_j (a(j) . b(j + lag))^2, lag = dw + kLagsPerLane l16 + d,
// j + lag < F.  float32 dot products; float32 partial sums, 4 independent accumulators per lag, at most 16 terms each, folded into
// float64 every kFlush steps.  The accumulators start at -center, which the fold adds back exactly: kCenter for unit vectors, whose
// terms are close to 1; a caller whose terms are smaller (k_ct_dipolar, sr_ct_dipolar.hip) passes half of what 16 of them come to.
__device__ __forceinline__ void ct_shift_block(const float *la, const float *lb, int Hf, int F, int dw, int g, int l16,
                                               double (&acc64)[kLagsPerLane], const float center = kCenter)
{
    const int nj = F - dw;
    const int S = (((nj + 3) >> 2) + 15) & ~15;        // strip length, multiple of 16: an even number of steps
    const int iters = S >> 3;
    const float *pa0 = la + ((g * S) >> 3) * 12;                              // even chunks of the a window
    const float *pa1 = pa0 + Hf;                                               // odd chunks
    const float *pb0 = lb + ((g * S + dw + kLagsPerLane * l16) >> 3) * 12;    // even chunks of the b window
    const float *pb1 = pb0 + Hf;

    // The 16-frame b window of a step is [P | Q]: P = its first 8 frames, Q = the next 8.  The following step's
    // window starts 8 frames later, i.e. with this step's Q -- so only ONE new half is read per step and the two
    // halves swap roles (12 instead of 18 ds_read_b128 per 256 FMAs).
    float Px[8], Py[8], Pz[8], Qx[8], Qy[8], Qz[8];
#define SR_CT_LOAD_HALF(HX, HY, HZ, OFF)                                                         \
    {                                                                                        \
        const float4 t0 = *reinterpret_cast<const float4 *>(pb0 + (OFF));                   \
        const float4 t1 = *reinterpret_cast<const float4 *>(pb0 + (OFF) + 4);               \
        const float4 t2 = *reinterpret_cast<const float4 *>(pb0 + (OFF) + 8);               \
        const float4 u0 = *reinterpret_cast<const float4 *>(pb1 + (OFF));                   \
        const float4 u1 = *reinterpret_cast<const float4 *>(pb1 + (OFF) + 4);               \
        const float4 u2 = *reinterpret_cast<const float4 *>(pb1 + (OFF) + 8);               \
        HX[0] = t0.x; HX[1] = t0.y; HX[2] = t0.z; HX[3] = t0.w; HX[4] = u0.x; HX[5] = u0.y; HX[6] = u0.z; HX[7] = u0.w; \
        HY[0] = t1.x; HY[1] = t1.y; HY[2] = t1.z; HY[3] = t1.w; HY[4] = u1.x; HY[5] = u1.y; HY[6] = u1.z; HY[7] = u1.w; \
        HZ[0] = t2.x; HZ[1] = t2.y; HZ[2] = t2.z; HZ[3] = t2.w; HZ[4] = u2.x; HZ[5] = u2.y; HZ[6] = u2.z; HZ[7] = u2.w; \
    }
#define SR_CT_STEP(LX, LY, LZ, HX, HY, HZ)                                                       \
    {                                                                                        \
        float ax[kJT], ay[kJT], az[kJT], bx[16], by[16], bz[16];                             \
        {                                                                                    \
            const float4 tx = *reinterpret_cast<const float4 *>(pa0);                       \
            const float4 ty = *reinterpret_cast<const float4 *>(pa0 + 4);                   \
            const float4 tz = *reinterpret_cast<const float4 *>(pa0 + 8);                   \
            const float4 ux = *reinterpret_cast<const float4 *>(pa1);                       \
            const float4 uy = *reinterpret_cast<const float4 *>(pa1 + 4);                   \
            const float4 uz = *reinterpret_cast<const float4 *>(pa1 + 8);                   \
            ax[0] = tx.x; ax[1] = tx.y; ax[2] = tx.z; ax[3] = tx.w; ax[4] = ux.x; ax[5] = ux.y; ax[6] = ux.z; ax[7] = ux.w; \
            ay[0] = ty.x; ay[1] = ty.y; ay[2] = ty.z; ay[3] = ty.w; ay[4] = uy.x; ay[5] = uy.y; ay[6] = uy.z; ay[7] = uy.w; \
            az[0] = tz.x; az[1] = tz.y; az[2] = tz.z; az[3] = tz.w; az[4] = uz.x; az[5] = uz.y; az[6] = uz.z; az[7] = uz.w; \
        }                                                                                    \
        SR_CT_LOAD_HALF(HX, HY, HZ, 12)                                                      \
        _Pragma("unroll") for (int t = 0; t < 8; ++t) {                                      \
            bx[t] = LX[t]; by[t] = LY[t]; bz[t] = LZ[t];                                     \
            bx[8 + t] = HX[t]; by[8 + t] = HY[t]; bz[8 + t] = HZ[t];                         \
        }                                                                                    \
        _Pragma("unroll") for (int jj = 0; jj < kJT; ++jj) {                                 \
            _Pragma("unroll") for (int d = 0; d < kLagsPerLane; ++d) {                       \
                float dot = ax[jj] * bx[jj + d];                                             \
                dot = fmaf(ay[jj], by[jj + d], dot);                                         \
                dot = fmaf(az[jj], bz[jj + d], dot);                                         \
                acc[d][jj & 3] = fmaf(dot, dot, acc[d][jj & 3]);                             \
            }                                                                                \
        }                                                                                    \
        pa0 += 12; pa1 += 12; pb0 += 12; pb1 += 12;                                          \
    }
    SR_CT_LOAD_HALF(Px, Py, Pz, 0)
    for (int it0 = 0; it0 < iters; it0 += kFlush) {
        float acc[kLagsPerLane][4];
#pragma unroll
        for (int d = 0; d < kLagsPerLane; ++d)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[d][q] = -center;
        const int n = min(kFlush, iters - it0);            // even
        for (int ii = 0; ii < n; ii += 2) {
            SR_CT_STEP(Px, Py, Pz, Qx, Qy, Qz)
            SR_CT_STEP(Qx, Qy, Qz, Px, Py, Pz)
        }
#pragma unroll
        for (int d = 0; d < kLagsPerLane; ++d) {
            const float s = (acc[d][0] + acc[d][1]) + (acc[d][2] + acc[d][3]);
            acc64[d] += (double)s + 4.0 * (double)center;
        }
    }
#undef SR_CT_STEP
#undef SR_CT_LOAD_HALF
}

// combine the 4 j strips: the lanes of strip 0 collect the partial sums of strips 1..3
__device__ __forceinline__ void ct_combine_strips(double (&acc64)[kLagsPerLane], int l16)
{
    const int s1 = strip_to_lane(1, l16), s2 = strip_to_lane(2, l16), s3 = strip_to_lane(3, l16);
#pragma unroll
    for (int d = 0; d < kLagsPerLane; ++d) {
        const double v0 = acc64[d];
        const double v1 = __shfl(v0, s1, 64), v2 = __shfl(v0, s2, 64), v3 = __shfl(v0, s3, 64);
        acc64[d] = (v0 + v1) + (v2 + v3);
    }
}

}  // namespace
