// sr_ct_direct.hip -- kernel 1, direct form: the Palmer-chunked P2 autocorrelation by shifted products (k_ct_palmer), float32 dot
// products (or float64 throughout in the validation mode).  Which chunks take it: the dispatch of sr_ct.hip.
//
// Reference semantics: calculate_Ct_Palmer, calculate-Ct-from-traj.py:200-238 (see include/spinrelax_hip.h).
//
// Direct kernel design:
//   * one workgroup stages ONE (chunk r, vector v) time series of F frames into LDS as three float
//     planes (x, y, z) -- 48 KB at F = 4096, so three workgroups share a CU's 160 KB;
//   * the (j, lag) plane is cut into lag blocks of 128 lags; a wave owns a lag block, its 64 lanes
//     are 4 j-strips x 16 lag-lanes, each lag-lane owns 8 consecutive lags.  Per step a lane needs
//     8 a-values and a 16-frame b window per component and issues 8x8x4 = 256 FMAs (3 for u(j).u(j+lag), 1 for
//     the square-accumulate).  Consecutive steps' b windows overlap by 8 frames: the window is kept as two
//     8-frame halves that swap roles, so a step reads 6 + 6 = 12 ds_read_b128 (18 without the rotation);
//   * LDS layout is "chunk-parity split, xyz-interleaved": 16-byte chunk c (4 frames of one component) lives
//     in half (c & 1) at slot (c >> 1); a slot is 48 bytes = [x-chunk | y-chunk | z-chunk].  Lag-lanes whose
//     windows start 8 floats (2 chunks) apart therefore read slots 48 bytes apart -- 3*l mod 16 is a
//     permutation, so the 16 lanes of a ds_read_b128 group hit 16 different 16-byte bank groups -- and all
//     18 reads of a step use immediate offsets from four base registers;
//   * the 64 lanes are mapped to (strip, lag-lane) along the hardware's ds_read_b128 lane groups
//     {0-3,12-15,20-27} {4-11,16-19,28-31} {32-35,44-47,52-59} {36-43,48-51,60-63} (MI355X_MICROARCH.md,
//     LDS): every group belongs to ONE strip, so its a-window read is a broadcast and its b-window reads are
//     conflict-free for any strip length;
//   * partial sums: float32, 4 independent accumulators per lag, at most 16 terms each, folded into
//     float64 every 8 steps; strips are combined with two float64 wave shuffles; no atomics;
//   * lags that do not fill a 128-lag block (for F = 4096 only lag 2048) and the validation mode run
//     through a simple float64 path in the same launch.
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

// ------------------------------------------------------------------------------------------
// kernel 1
// ------------------------------------------------------------------------------------------
struct CtArgs {
    const float *soa;
    int64_t Npad;
    const int64_t *chunk_start;   // device, may be null
    double *psum;                 // (nV, R, Lp)
    int R, F, Fp, L, Lp, nslab, mode;
};

#ifndef SR_CT_WAVES_EU
#define SR_CT_WAVES_EU 3
#endif
template <int W>
__global__ __launch_bounds__(W * 64, SR_CT_WAVES_EU) void k_ct_palmer(CtArgs a)
{
    extern __shared__ __align__(16) float lds[];
    // This is the throughput kernel of the pipeline; the fit wavefronts of the previous batch share its SIMDs.  Raised
    // issue priority makes them fill the slots this kernel leaves idle instead of taking turns with it.
    __builtin_amdgcn_s_setprio(3);
    const int Fp = a.Fp, Hf = (Fp >> 3) * 12, F = a.F;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int series = blockIdx.x / a.nslab;
    const int slab = blockIdx.x - series * a.nslab;
    const int v = series / a.R;
    const int r = series - v * a.R;

    // ---- stage the series (coalesced dword loads; zero padding behind frame F) ----
    {
        const int64_t start = a.chunk_start ? a.chunk_start[r] : (int64_t)r * F;
        const float *px = a.soa + ((int64_t)v * 3 + 0) * a.Npad + start;
        const float *py = px + a.Npad;
        const float *pz = py + a.Npad;
        for (int e = tid; e < Fp; e += W * 64) {
            const int p = lds_pos(e, 0, Hf);
            const bool in = e < F;
            lds[p] = in ? px[e] : 0.f;
            lds[p + 4] = in ? py[e] : 0.f;
            lds[p + 8] = in ? pz[e] : 0.f;
        }
    }
    __syncthreads();

    const int NW = a.nslab * W;            // workers (waves) per series
    const int wid = slab * W + wave;
    double *out = a.psum + ((int64_t)v * a.R + r) * a.Lp;
    const int nb = (a.mode == 0) ? (a.L + 1) / kLagBlock : 0;

    // ---- fast path: full lag blocks, serpentine assignment balances the (F - lag) work ----
    int g, l16;
    lane_to_strip(lane, g, l16);
    for (int i = 0; i * NW < nb; ++i) {
        const int k = (i & 1) ? i * NW + (NW - 1 - wid) : i * NW + wid;
        if (k >= nb) continue;
        const int dw = k * kLagBlock;
        const int nj = F - dw;
        const int S = (((nj + 3) >> 2) + 15) & ~15;        // strip length, multiple of 16: an even number of steps
        const int iters = S >> 3;
        const float *pa0 = lds + ((g * S) >> 3) * 12;                              // even chunks of the a window
        const float *pa1 = pa0 + Hf;                                               // odd chunks
        const float *pb0 = lds + ((g * S + dw + kLagsPerLane * l16) >> 3) * 12;    // even chunks of the b window
        const float *pb1 = pb0 + Hf;
        double acc64[kLagsPerLane];
#pragma unroll
        for (int d = 0; d < kLagsPerLane; ++d) acc64[d] = 0.0;

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
                for (int q = 0; q < 4; ++q) acc[d][q] = -kCenter;
            const int n = min(kFlush, iters - it0);            // even
            for (int ii = 0; ii < n; ii += 2) {
                SR_CT_STEP(Px, Py, Pz, Qx, Qy, Qz)
                SR_CT_STEP(Qx, Qy, Qz, Px, Py, Pz)
            }
#pragma unroll
            for (int d = 0; d < kLagsPerLane; ++d) {
                const float s = (acc[d][0] + acc[d][1]) + (acc[d][2] + acc[d][3]);
                acc64[d] += (double)s + 4.0 * (double)kCenter;
            }
        }
#undef SR_CT_STEP
#undef SR_CT_LOAD_HALF
        // combine the 4 j strips: the lanes of strip 0 collect the partial sums of strips 1..3
        {
            const int s1 = strip_to_lane(1, l16), s2 = strip_to_lane(2, l16), s3 = strip_to_lane(3, l16);
#pragma unroll
            for (int d = 0; d < kLagsPerLane; ++d) {
                const double v0 = acc64[d];
                const double v1 = __shfl(v0, s1, 64), v2 = __shfl(v0, s2, 64), v3 = __shfl(v0, s3, 64);
                acc64[d] = (v0 + v1) + (v2 + v3);
            }
        }
        if (g == 0) {
            double *o = out + dw + kLagsPerLane * l16;
#pragma unroll
            for (int d = 0; d < kLagsPerLane; ++d) o[d] = acc64[d];
        }
    }

    // ---- float64 path: remaining lags (and every lag in validation mode) ----
    {
        int lo = nb * kLagBlock;
        if (lo < 1) lo = 1;
        for (int d = lo + wid; d <= a.L; d += NW) {
            double s = 0.0;
            for (int j = lane; j + d < F; j += 64) {
                const int pa = lds_pos(j, 0, Hf), pb = lds_pos(j + d, 0, Hf);
                const double x = (double)lds[pa] * (double)lds[pb] + (double)lds[pa + 4] * (double)lds[pb + 4] +
                                 (double)lds[pa + 8] * (double)lds[pb + 8];
                s += x * x;
            }
            s = wave_sum_f64(s);
            if (lane == 0) out[d] = s;
        }
    }
}

template <int W>
int launch_ct(sr_ctx *ctx, const CtArgs &a, int64_t nblocks, size_t lds_bytes)
{
    return sr_launch(ctx, k_ct_palmer<W>, dim3((unsigned)nblocks), dim3(W * 64), lds_bytes, a);
}

}  // namespace

// the direct kernel stages a whole series in LDS: 12 bytes per frame
size_t sr_ct_direct_lds_bytes(int64_t F) { return (size_t)ct_Fp(F) * 3 * sizeof(float); }

int64_t sr_ct_direct_max_frames(size_t lds_limit)
{
    int64_t F = (int64_t)lds_limit / 12 - kPad - 64;
    return F > 0 ? F : 0;
}

// Called by sr_ct_palmer_sums_f32_dev (sr_ct.hip), which has checked that the series fits the LDS.
int sr_launch_ct_direct(sr_ctx *ctx, const sr_ct_job &j, int mode)
{
    CtArgs a;
    a.soa = j.soa; a.Npad = j.Npad; a.chunk_start = j.cs_dev; a.psum = j.psum;
    a.R = j.R; a.F = j.F; a.Fp = (int)ct_Fp(j.F); a.L = j.L; a.Lp = j.Lp; a.mode = mode;
    const size_t lds_bytes = sr_ct_direct_lds_bytes(j.F);
    const int nb = mode == 0 ? (j.L + 1) / kLagBlock : 0;
    if (mode == 1) {
        a.nslab = 1;
        return launch_ct<4>(ctx, a, j.series, lds_bytes);
    }
    if (nb >= 16) {
        a.nslab = nb >= 64 ? nb / 32 : 1;            // about 4-8 lag blocks per wave
        return launch_ct<4>(ctx, a, j.series * a.nslab, lds_bytes);
    }
    a.nslab = nb > 0 ? nb : 1;                       // one wave per workgroup, one lag block per wave
    return launch_ct<1>(ctx, a, j.series * a.nslab, lds_bytes);
}
