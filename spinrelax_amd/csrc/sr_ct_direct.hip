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
// The layout, the lane map and the lag-block loop are in sr_ct_shift.h; the workers, the serpentine, the float64 path and the launch
// ladder, which the other staged kernels share, in sr_ct_staged.h.
//
// Kernels:
//   k_ct_palmer<W>  one (vector, chunk) per workgroup of W waves or per slab of one; lags 1 .. L (slot 0 of a psum row stays unused)
#include "sr_ct_staged.h"

namespace {

// ------------------------------------------------------------------------------------------
// kernel 1
// ------------------------------------------------------------------------------------------
#ifndef SR_CT_WAVES_EU
#define SR_CT_WAVES_EU 3
#endif
template <int W>
__global__ __launch_bounds__(W * 64, SR_CT_WAVES_EU) void k_ct_palmer(CtStagedArgs a)
{
    extern __shared__ __align__(16) float lds[];
    // This is the throughput kernel of the pipeline; the fit wavefronts of the previous batch share its SIMDs.  Raised
    // issue priority makes them fill the slots this kernel leaves idle instead of taking turns with it.
    __builtin_amdgcn_s_setprio(3);
    const int Fp = a.Fp, Hf = (Fp >> 3) * 12, F = a.F;
    const CtWorker w = ct_worker<W>(a, a.nslab);
    const int tid = w.tid, lane = w.lane;

    // ---- stage the series (coalesced dword loads; zero padding behind frame F) ----
    {
        const float *px = a.soa + ((int64_t)w.row * 3 + 0) * a.Npad + ct_chunk_start(a, w);
        const float *py = px + a.Npad;
        const float *pz = py + a.Npad;
        ct_stage_series<W * 64>(lds, px, py, pz, F, Fp, Hf, tid);
    }
    __syncthreads();

    const int NW = ct_workers<W>(a.nslab), wid = ct_worker_id<W>(w);
    double *out = ct_psum_row(a, w, a.Lp);
    const int nb = ct_full_blocks(a);

    // ---- fast path: full lag blocks, serpentine assignment balances the (F - lag) work.  This loop and the next are those of
    // ct_for_each_lag_block and ct_tail_lags (sr_ct_staged.h), written out: through the helpers the compiler lays the same instructions
    // out in another order, and this kernel's code object is held to "same" from revision to revision (scripts/dev/isa_diff.py) ----
    int g, l16;
    lane_to_strip(lane, g, l16);
    for (int i = 0; i * NW < nb; ++i) {
        const int k = ct_serpentine(i, NW, wid);
        if (k >= nb) continue;
        const int dw = k * kLagBlock;
        double acc64[kLagsPerLane];
        ct_zero_lags(acc64);
        ct_shift_block(lds, lds, Hf, F, dw, g, l16, acc64);
        ct_combine_strips(acc64, l16);
        if (g == 0) {
            double *o = out + dw + kLagsPerLane * l16;
#pragma unroll
            for (int d = 0; d < kLagsPerLane; ++d) o[d] = acc64[d];
        }
    }

    // ---- float64 path: remaining lags (and every lag in validation mode), from lag 1: slot 0 of a psum row stays unused ----
    for (int d = max(nb * kLagBlock, 1) + wid; d <= a.L; d += NW) {
        double s = 0.0;
        for (int j = lane; j + d < F; j += 64) {
            const int pa = lds_pos(j, 0, Hf), pb = lds_pos(j + d, 0, Hf);
            const double x = ct_dot_f64(lds, lds, pa, pb);
            s += x * x;
        }
        s = wave_sum_f64(s);
        if (lane == 0) out[d] = s;
    }
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
    CtStagedArgs a = ct_staged_args(j.soa, j.Npad, j.cs_dev, j.psum, j.R, j.F, mode);
    return ct_launch_slabs(ctx, k_ct_palmer<1>, k_ct_palmer<4>, a, j.series, 12);
}
