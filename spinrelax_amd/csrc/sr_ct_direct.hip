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
// The layout, the lane map and the lag-block loop are in sr_ct_shift.h: k_ct_cross (sr_ct_cross.hip) runs them on two series.
#include "sr_ct_shift.h"

namespace {

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
        ct_stage_series<W * 64>(lds, px, py, pz, F, Fp, Hf, tid);
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
        double acc64[kLagsPerLane];
#pragma unroll
        for (int d = 0; d < kLagsPerLane; ++d) acc64[d] = 0.0;
        ct_shift_block(lds, lds, Hf, F, dw, g, l16, acc64);
        ct_combine_strips(acc64, l16);
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
