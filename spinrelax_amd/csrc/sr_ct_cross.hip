// sr_ct_cross.hip -- time-lagged P2 cross-correlation between pairs of bond vectors (k_ct_cross), an extension beyond the
// reference, which only ever correlates a vector with itself:
//     S_ij[k] = sum_{t=0}^{F-1-k} (u_i(t) . u_j(t+k))^2,   k = 0 .. L = F/2,   per (pair p = (i, j), chunk r)
// on the Palmer chunk table of kernel 1.  Lags 1 .. L leave as raw sums in kernel 1's layout (pair, chunk, sr_ct_psum_stride(F)) --
// pairs in the place of vectors -- so k_ct_finalize (sr_ct.hip) turns them into C(t) = mean over chunks of 1.5 S / (F - k) - 0.5 and
// dC(t) unchanged.  Lag 0, the equal-time <P2(u_i . u_j)> (the rigid-limit P2(cos theta_ij)), sits in slot 0 of the same rows, which
// the finalizer skips; k_ct_cross_p0 averages it over the chunks.
//
// Design:
//   * one workgroup of 8 waves stages BOTH series of one (pair, chunk) in LDS in the layout of the direct kernel (sr_ct_shift.h):
//     24 bytes per frame, 101 KB at F = 4096 -- one workgroup per CU, hence 8 waves and not the direct kernel's 4 (at 150 VGPRs a
//     SIMD holds 3 waves, so a CU holds one such workgroup whatever F is: 8 waves per CU against the direct kernel's 12);
//   * a wave owns a block of 128 lags and runs the direct kernel's lag-block loop on it, a from series i and b from series j for
//     S_ij; in the symmetric form (sym = 1, what relaxation theory uses) the same wave runs the loop a second time with the series
//     exchanged and writes (S_ij + S_ji) / 2: both directions of a lag are summed by one lane in a fixed order, so there are no
//     atomics and the bits do not change from run to run.  For i = j the symmetric sum is the autocorrelation's, to rounding;
//   * serpentine assignment of the lag blocks to the waves as in the direct kernel (at F = 4096: 16 blocks, two per wave, equal work);
//   * lags that do not fill a block, and every lag in the validation mode (mode 1), take a float64 path in the same launch.
// A chunk whose two series do not fit the LDS is refused here (sr_ct_cross_max_frames); the entry points sr_*ct_cross_long_* give such
// chunks to the blocked form (sr_ct_cross_long.hip).
// The workers, the serpentine, the float64 path and the argument struct: sr_ct_staged.h.
//
// Kernels:
//   k_ct_cross     one (pair, chunk) per workgroup of 8 waves; lags 0 .. L
//   k_ct_cross_p0  the equal-time value and its error from slot 0 of the raw sums
#include "sr_ct_staged.h"

namespace {

constexpr int kCrossWaves = 8;

__global__ __launch_bounds__(kCrossWaves * 64, 2) void k_ct_cross(CtStagedArgs a)
{
    extern __shared__ __align__(16) float lds[];
    const int Fp = a.Fp, Hf = (Fp >> 3) * 12, F = a.F;
    const CtWorker w = ct_worker<kCrossWaves>(a, 1);
    const int tid = w.tid, lane = w.lane, p = w.row;
    float *si = lds, *sj = lds + 2 * Hf;

    // ---- stage the two series ----
    {
        const int64_t start = ct_chunk_start(a, w);
        const float *pi = a.soa + (int64_t)a.pair_i[p] * 3 * a.Npad + start;
        const float *pj = a.soa + (int64_t)a.pair_j[p] * 3 * a.Npad + start;
        ct_stage_series<kCrossWaves * 64>(si, pi, pi + a.Npad, pi + 2 * a.Npad, F, Fp, Hf, tid);
        ct_stage_series<kCrossWaves * 64>(sj, pj, pj + a.Npad, pj + 2 * a.Npad, F, Fp, Hf, tid);
    }
    __syncthreads();

    const int NW = ct_workers<kCrossWaves>(1), wid = ct_worker_id<kCrossWaves>(w);
    double *out = ct_psum_row(a, w, a.Lp);
    const int nb = ct_full_blocks(a);
    const int sym = a.sym;
    const double scale = sym ? 0.5 : 1.0;

    // ---- fast path: full lag blocks (lag 0 included) ----
    ct_for_each_lag_block(nb, NW, wid, lane, [=](int dw, int g, int l16) SR_CT_INLINE {
        double acc64[kLagsPerLane];
        ct_zero_lags(acc64);
        ct_shift_block(si, sj, Hf, F, dw, g, l16, acc64);                 // S_ij
        if (sym) ct_shift_block(sj, si, Hf, F, dw, g, l16, acc64);        // + S_ji
        ct_combine_strips(acc64, l16);
        if (g == 0) {
            double *o = ct_lag_slots(out, dw, l16);
#pragma unroll
            for (int d = 0; d < kLagsPerLane; ++d) o[d] = scale * acc64[d];
        }
    });

    // ---- float64 path: remaining lags (and every lag in validation mode) ----
    ct_tail_lags<1>(nb * kLagBlock, a.L, F, NW, wid, lane, [=](int t, int d, double (&s)[1]) SR_CT_INLINE {
        const int pa = lds_pos(t, 0, Hf), pb = lds_pos(t + d, 0, Hf);
        const double x = ct_dot_f64(si, sj, pa, pb);
        s[0] += x * x;
        if (sym) {
            const double y = ct_dot_f64(sj, si, pa, pb);
            s[0] += y * y;
        }
    }, [=](int d, const double (&s)[1]) SR_CT_INLINE { out[d] = scale * s[0]; });
}

// P0[p] = mean over the chunks of 1.5 S[p][r][0] / F - half (half: k_ct_finalize's), summed in chunk order; dP0[p] (may be null) = their two-pass standard
// deviation / (sqrt(R) - 1), the formula of k_ct_finalize
__global__ __launch_bounds__(256) void k_ct_cross_p0(const double *__restrict__ psum, int R, int F, int Lp, int64_t nP, double half,
                                                     double *__restrict__ P0, double *__restrict__ dP0)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nP) return;
    const double *s = psum + p * R * Lp;
    double m = 0.0;
    for (int r = 0; r < R; ++r) m += 1.5 * (s[(int64_t)r * Lp] / (double)F) - half;
    m /= (double)R;
    P0[p] = m;
    if (!dP0) return;
    double v = 0.0;
    for (int r = 0; r < R; ++r) {
        const double e = (1.5 * (s[(int64_t)r * Lp] / (double)F) - half) - m;
        v += e * e;
    }
    dP0[p] = sqrt(v / (double)R) / (sqrt((double)R) - 1.0);
}

}  // namespace

int sr_ct_cross_p0_dev(sr_ctx *ctx, const double *psum, int64_t R, int64_t F, int64_t nP, double half, double *P0, double *dP0)
{
    hipLaunchKernelGGL(k_ct_cross_p0, dim3((unsigned)((nP + 255) / 256)), dim3(256), 0, ctx->stream, psum, (int)R, (int)F,
                       (int)sr_ct_psum_stride(F), nP, half, P0, dP0);
    SR_HIP(hipGetLastError());
    return 0;
}

extern "C" {

int64_t sr_ct_cross_max_frames(sr_ctx *ctx)
{
    if (!ctx) return -1;
    return sr_ct_lds_max_frames(sr_ct_form_cross.bytes_per_frame, sr_lds_limit(ctx));
}

static int cross_f32_dev(sr_ctx *ctx, const char *who, int blocked, const float *soa, int64_t Npad, int64_t nV, int64_t R, int64_t F,
                         const int64_t *chunk_start_host, const int32_t *pair_i_host, const int32_t *pair_j_host, int64_t nP, int sym, int mode,
                         double *psum_ws, double *P0, double *dP0, double *Ct, double *dCt)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(soa && P0 && Ct && dCt, -2, "%s: null pointer", who);
    const sr_ct_rows w = {who, Npad, nV, R, F, chunk_start_host, pair_i_host, pair_j_host, nP, sym, mode, blocked};
    if (int rc = sr_ct_rows_check(ctx, w, sr_ct_form_cross)) return rc;
    const int64_t L = F / 2, Lp = sr_ct_psum_stride(F);
    double *psum = sr_ct_psum(ctx, psum_ws, nP, R, F);
    if (!psum) return -5;
    sr_stage st(ctx);
    const sr_ct_tables t = sr_ct_stage_tables(st, w, blocked ? 2 * (size_t)nP * sizeof(int32_t) : 0);
    if (blocked) {
        const sr_ct_pair_job job = {{soa, Npad, chunk_start_host, t.chunk_start, psum, (int)R, (int)F, (int)L, (int)Lp, R * nP},
                                    nV, nP, pair_i_host, pair_j_host, t.pair_i, t.pair_j, sym, mode, &st};
        if (int rc = sr_launch_ct_cross_long(ctx, job)) return rc;
    } else {
        if (int rc = st.finish()) return rc;            // small tables: the caller's arrays are free again when this returns
        CtStagedArgs a = ct_staged_args(soa, Npad, t.chunk_start, psum, R, F, mode);
        a.pair_i = t.pair_i; a.pair_j = t.pair_j; a.sym = sym;
        if (int rc = sr_launch(ctx, k_ct_cross, dim3((unsigned)(nP * R)), dim3(kCrossWaves * 64),
                               sr_ct_lds_bytes(F, sr_ct_form_cross.bytes_per_frame), a))
            return rc;
    }
    if (int rc = sr_ct_cross_p0_dev(ctx, psum, R, F, nP, 0.5, P0, dP0)) return rc;
    return sr_ct_finalize_f64_dev(ctx, psum, R, F, nP, Ct, dCt);
}

int sr_ct_cross_f32_dev(sr_ctx *ctx, const float *soa, int64_t Npad, int64_t nV, int64_t R, int64_t F, const int64_t *chunk_start_host,
                        const int32_t *pair_i_host, const int32_t *pair_j_host, int64_t nP, int sym, int mode, double *psum_ws,
                        double *P0, double *dP0, double *Ct, double *dCt)
{
    return cross_f32_dev(ctx, "sr_ct_cross_f32_dev", 0, soa, Npad, nV, R, F, chunk_start_host, pair_i_host, pair_j_host, nP, sym, mode, psum_ws, P0,
                         dP0, Ct, dCt);
}

int64_t sr_ct_cross_long_max_frames(sr_ctx *ctx)
{
    if (!ctx) return -1;
    return SR_CT_LONG_MAX_FRAMES;
}

int sr_ct_cross_long_f32_dev(sr_ctx *ctx, const float *soa, int64_t Npad, int64_t nV, int64_t R, int64_t F, const int64_t *chunk_start_host,
                             const int32_t *pair_i_host, const int32_t *pair_j_host, int64_t nP, int sym, int mode, double *psum_ws,
                             double *P0, double *dP0, double *Ct, double *dCt)
{
    return cross_f32_dev(ctx, "sr_ct_cross_long_f32_dev", 1, soa, Npad, nV, R, F, chunk_start_host, pair_i_host, pair_j_host, nP, sym, mode, psum_ws,
                         P0, dP0, Ct, dCt);
}

}  // extern "C"
