// sr_ct_staged.h -- what the five staged correlation kernels have in common around their inner loops: k_ct_palmer (sr_ct_direct.hip),
// k_ct_cross (sr_ct_cross.hip), k_ct_dipolar (sr_ct_dipolar.hip), k_ct_dipolar_cross (sr_ct_dipolar_cross.hip) and k_ct_modes
// (sr_ct_modes.hip).  Each stages the series of one row -- a vector or a pair of vectors -- and one chunk of kernel 1's Palmer chunk
// table in LDS, runs shifted-product lag blocks over them (ct_shift_block, sr_ct_shift.h; dip_shift_block_w, sr_ct_dipolar.h) and
// leaves raw lag sums in kernel 1's psum layout.  Said here once, for all five:
//   * a launch: one argument struct (CtStagedArgs); blockIdx.x = (row * R + chunk) * nslab + slab, and the workgroups ("slabs") of one
//     (row, chunk) stage the same series and share its lag blocks.  Workers are waves: NW = nslab * W per series, wave `wave` of slab
//     `slab` is worker wid = slab * W + wave (the two 8-wave pair kernels have nslab = 1 at compile time: NW = 8, wid = wave);
//   * nb = (L + 1) / kLagBlock full blocks of 128 lags in mode 0, none in the validation mode (mode 1);
//   * the fast path (ct_for_each_lag_block): worker wid takes block i NW + wid on even passes i and block i NW + (NW - 1 - wid) on odd
//     ones -- a block's work falls with its lag as F - lag, and the serpentine gives every worker about the same; a kernel's body for
//     one block zeroes its float64 accumulators (ct_zero_lags), runs its shift blocks, combines the four j strips (ct_combine_strips)
//     and has the lanes of strip 0 store what they then hold, eight consecutive lags per lane (ct_lag_slots);
//   * the float64 path (ct_tail_lags): the lags behind the last full block and every lag in mode 1, lag lo + wid, + NW, ... per
//     worker, a wave per lag, the lanes 64 frames apart, summed across the wave in a fixed order (wave_sum_f64), stored by lane 0;
//   * the launch ladder (ct_launch_slabs): which of the W = 1 and W = 4 instances runs and how many slabs.
// No atomics anywhere: equal input gives bit-equal output.  A kernel's own file says how it stages its series, what it computes before
// the lag blocks, which shift blocks make one lag block and how the sums combine, and its float64 term for one (frame, lag).
// k_ct_palmer writes the two loops out (why: at its loops); everything else here it uses like the other four.
#pragma once
#include "sr_ct_shift.h"

// on the lambdas given to ct_for_each_lag_block and ct_tail_lags: inlined with the helpers, before the compiler's first simplification
// of the kernel, as if written in place.  Left to the inliner's own turn they are simplified alone first, and the kernels come out
// with other register allocations (k_ct_dipolar<4>: one VGPR more)
#define SR_CT_INLINE __attribute__((always_inline))

namespace {

// The first eleven fields are k_ct_palmer's argument struct as it always was: its code object does not change.
struct CtStagedArgs {
    const float *soa;                 // the packed planes, Npad floats each
    int64_t Npad;
    const int64_t *chunk_start;       // device, may be null: chunk r starts at r F
    double *psum;                     // (rows, R, Lp); k_ct_modes: (rows, R, 6, Lp)
    int R, F, Fp, L, Lp, nslab, mode;
    int sym;                          // the pair kernels: 1 = the mean of both directions
    const int32_t *pair_i, *pair_j;   // the pair kernels: device, row p is the pair (pair_i[p], pair_j[p])
    double *sums;                     // the chunk sums a form leaves beside psum: wsum (k_ct_dipolar), wsum2 (k_ct_dipolar_cross), ssum (k_ct_modes)
};

// everything of the job but what a form adds (sym, the pair table, sums)
inline CtStagedArgs ct_staged_args(const float *soa, int64_t Npad, const int64_t *chunk_start_dev, double *psum, int64_t R, int64_t F, int mode)
{
    CtStagedArgs a = {};
    a.soa = soa; a.Npad = Npad; a.chunk_start = chunk_start_dev; a.psum = psum;
    a.R = (int)R; a.F = (int)F; a.Fp = (int)ct_Fp(F); a.L = (int)(F / 2); a.Lp = (int)sr_ct_psum_stride(F); a.nslab = 1; a.mode = mode;
    return a;
}

// who a thread is: its wave and lane, and the row (vector or pair), chunk and slab of its workgroup
struct CtWorker {
    int tid, lane, wave, row, r, slab;
};

// nslab: a.nslab for the kernels launched by ct_launch_slabs, the literal 1 for the pair kernels, whose grid is one workgroup per series
template <int W>
__device__ __forceinline__ CtWorker ct_worker(const CtStagedArgs &a, int nslab)
{
    CtWorker w;
    w.tid = threadIdx.x;
    w.lane = w.tid & 63;
    w.wave = __builtin_amdgcn_readfirstlane(w.tid >> 6);
    const int series = blockIdx.x / nslab;
    w.slab = blockIdx.x - series * nslab;
    w.row = series / a.R;
    w.r = series - w.row * a.R;
    return w;
}

// the waves that share the lags of one series, and this wave's number among them
template <int W>
__device__ __forceinline__ int ct_workers(int nslab) { return nslab * W; }
template <int W>
__device__ __forceinline__ int ct_worker_id(const CtWorker &w) { return w.slab * W + w.wave; }

// the worker's psum row; row_stride: doubles per (row, chunk)
__device__ __forceinline__ double *ct_psum_row(const CtStagedArgs &a, const CtWorker &w, int row_stride)
{
    return a.psum + ((int64_t)w.row * a.R + w.r) * row_stride;
}

// full lag blocks of a series: none in the validation mode
__device__ __forceinline__ int ct_full_blocks(const CtStagedArgs &a) { return (a.mode == 0) ? (a.L + 1) / kLagBlock : 0; }

// first frame of the worker's chunk
__device__ __forceinline__ int64_t ct_chunk_start(const CtStagedArgs &a, const CtWorker &w)
{
    return a.chunk_start ? a.chunk_start[w.r] : (int64_t)w.r * a.F;
}

__device__ __forceinline__ void ct_zero_lags(double (&acc64)[kLagsPerLane])
{
#pragma unroll
    for (int d = 0; d < kLagsPerLane; ++d) acc64[d] = 0.0;
}

// the lag block of worker wid in pass i: up the workers on even passes, down on odd ones
__device__ __forceinline__ int ct_serpentine(int i, int NW, int wid) { return (i & 1) ? i * NW + (NW - 1 - wid) : i * NW + wid; }

// block(dw, g, l16) for every full lag block of this worker: the block starts at lag dw, the lane is (strip g, lag-lane l16)
template <class Block>
__device__ __forceinline__ void ct_for_each_lag_block(int nb, int NW, int wid, int lane, Block block)
{
    int g, l16;
    lane_to_strip(lane, g, l16);
    for (int i = 0; i * NW < nb; ++i) {
        const int k = ct_serpentine(i, NW, wid);
        if (k >= nb) continue;
        block(k * kLagBlock, g, l16);
    }
}

// where lag-lane l16 stores its eight lags of the block at dw in the psum row `out`.  After ct_combine_strips the lanes of strip 0
// (g == 0) hold the sums, and only they store.  (The store itself stays in the kernels: a helper that takes the accumulators, as an
// array or in a closure, keeps them in memory through the compiler's early passes, and the lag-block loop comes out with more registers.)
__device__ __forceinline__ double *ct_lag_slots(double *out, int dw, int l16) { return out + (dw + kLagsPerLane * l16); }

// float64 a(j) . b(j + d) of two staged xyz series, pa = lds_pos(j, 0, Hf), pb = lds_pos(j + d, 0, Hf)
__device__ __forceinline__ double ct_dot_f64(const float *la, const float *lb, int pa, int pb)
{
    return (double)la[pa] * (double)lb[pb] + (double)la[pa + 4] * (double)lb[pb + 4] + (double)la[pa + 8] * (double)lb[pb + 8];
}

// lags lo .. L in float64: term(j, d, s) adds the term of frame j and lag d to the NS sums s; store(d, s), called on lane 0, gets
// their sums over the wave
template <int NS, class Term, class Store>
__device__ __forceinline__ void ct_tail_lags(int lo, int L, int F, int NW, int wid, int lane, Term term, Store store)
{
    for (int d = lo + wid; d <= L; d += NW) {
        double s[NS];
#pragma unroll
        for (int c = 0; c < NS; ++c) s[c] = 0.0;
        for (int j = lane; j + d < F; j += 64) term(j, d, s);
#pragma unroll
        for (int c = 0; c < NS; ++c) s[c] = wave_sum_f64(s[c]);
        if (lane == 0) store(d, s);
    }
}

// The launch ladder of the three forms that share a series among slabs: `series` = rows x R (row, chunk) series, k1 and k4 the form's
// W = 1 and W = 4 instances.  Sets a.nslab.
//   mode 1            W = 4, one workgroup per series: four waves share the float64 lags
//   nb >= 16          W = 4, one workgroup per series: at least 4 lag blocks per wave.  From 64 blocks on, slabs of 32 blocks each would
//                     keep that at 8, but nb >= 64 takes F >= 16382, and the longest chunk that fits 160 KiB of LDS has 13397 frames
//                     (k_ct_palmer, 12 bytes per frame), 10016 (k_ct_dipolar, 16) or 7968 (k_ct_modes, 20) -- sr_ct_lds_max_frames, to
//                     which sr_ct_rows_check and the dispatch of sr_ct_palmer_sums_f32_dev hold every launch: at most 52 blocks
//   nb < 16           W = 1, one workgroup (one wave) per lag block, or one per series where there is no full block
inline int ct_launch_slabs(sr_ctx *ctx, void (*k1)(CtStagedArgs), void (*k4)(CtStagedArgs), CtStagedArgs &a, int64_t series, int bytes_per_frame)
{
    const size_t lds_bytes = sr_ct_lds_bytes(a.F, bytes_per_frame);
    const int nb = a.mode == 0 ? (a.L + 1) / kLagBlock : 0;
    if (a.mode == 1 || nb >= 16) {
        a.nslab = 1;
        return sr_launch(ctx, k4, dim3((unsigned)series), dim3(4 * 64), lds_bytes, a);
    }
    a.nslab = nb > 0 ? nb : 1;
    return sr_launch(ctx, k1, dim3((unsigned)(series * a.nslab)), dim3(64), lds_bytes, a);
}

}  // namespace
