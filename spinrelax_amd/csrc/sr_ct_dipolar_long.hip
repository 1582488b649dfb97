// sr_ct_dipolar_long.hip -- the two distance-weighted correlation functions, C_dd(k) of sr_ct_dipolar.hip and the pair form C_ij(k) of
// sr_ct_dipolar_cross.hip, for chunks that do not fit the LDS of a workgroup: the blocked transforms of sr_ct_long.hip and
// sr_ct_cross_long.hip on the four-plane pack a_x, a_y, a_z, w of sr_pack_dipolar_f32_dev, up to SR_CT_LONG_MAX_FRAMES frames per chunk.
//
// The algebra.  The pack has a = u sqrt(w), so |a|^2 = w.  With Q = a (x) a - (|a|^2 / 3) I, the traceless part,
//     (a . a')^2 = Q : Q' + |a|^2 |a'|^2 / 3
//     1.5 (a . a')^2 - 0.5 w w' = 1.5 Q : Q' + 0.5 (|a|^2 |a'|^2 - w w') = 1.5 Q : Q'
// so the unnormalised function of a chunk is 1.5 sum Q : Q' / (F - k): the five traceless signals that the blocked kernels already
// transform, and nothing else -- no sixth signal, no eps = |a|^2 - 1 term.  In CtlConst terms nsig = 5, weps = 0 and
// Kc = 6 sum_c w_c m_c^2 without the 1/3 per product of unit vectors: the raw sum is S' = sum Q : Q' = S_a - S_w / 3, what
// k_ct_dipolar leaves, and k_ct_finalize with half = 0 gives [1.5 S_a - 0.5 S_w] / (F - k).  The same holds term by term for a pair:
// 1.5 (a_i . a_j')^2 - 0.5 w_i w_j' = 1.5 Q_i : Q_j'.  The shared kernels take this as their "traceless" flag and the plane stride 4
// (CtlArgs / CtlxArgs, sr_ct_long.h).
//
// |a|^2 and w agree to the float32 rounding of the pack only (relative 1e-7 per frame, not systematic): on the test vectors the
// five-signal form differs from the definition on the same planes by 1.5e-9 of C (docs/EXPERIMENTS.md) -- on wobbling pairs whose w
// stays within a factor 3; on mobile pairs whose w spans four decades (docs/EXPERIMENTS.md section 38) mode 0 as a whole is within 1.6e-7
// of max(1, max |C|) on C and 2.1e-7 / (sqrt(R) - 1) on dC, at most 2.3 times an independent float32 emulation.  The planes must therefore
// come from sr_pack_dipolar_f32_dev; four planes whose first three are not sqrt(w) long give Q : Q', not the definition.
//
// What is not a transform stays the definition on the w plane, in float64, in a fixed order: the chunk sums of w and w^2 that
// normalise the function and give the distance outputs (k_dipl_wsums), and lag 0 of a pair (k_ctlx_scan).  Mode 1 (k_dipl_f64) is the
// definition from the planes, S_a and S_w separately, one thread per lag with the frames in order: the on-device check, not built for
// speed.  No atomics anywhere: equal input gives bit-equal output for any tiling of the work area.
//
// Launches of mode 0, autocorrelation: k_dipl_wsums, then sr_launch_ct_long (k_ctl_consts, k_ctl_scan, per tile k_ctl_spectra, k_ctl_cross,
// k_ctl_inverse), k_ct_finalize, k_ct_dipolar_norm.  Pair form: k_dipl_wsums, sr_launch_ct_cross_long (k_ctl_consts, k_ctlx_scan, per tile
// k_ctl_spectra, k_ctlx_cross, k_ctl_inverse), k_ct_cross_p0, k_ct_finalize, k_ct_dipolar_cross_norm.
#include "sr_internal.h"

namespace {

struct DiplArgs {
    const float *soa;                    // (nV, 4, Npad)
    int64_t Npad;
    const int64_t *chunk_start;          // device, may be null
    const int32_t *pair_i, *pair_j;      // device, [rows]; null: row v is vector v against itself
    double *psum;                        // (rows, R, Lp)
    double *wsum;                        // (rows, R, 2)
    int R, F, L, Lp, sym;
};

// ---- chunk sums of the w plane, float64 -----------------------------------------------------------------------------------------
// One workgroup per (row, chunk).  Autocorrelation form: sum of w and of w^2 (the wsum layout k_ct_dipolar_norm reads); pair form: sum of
// w_i^2 and of w_j^2 (wsum2 of k_ct_dipolar_cross_norm).  Thread t adds frames t, t + 256, ... in order, then the wave, then the four
// waves in order.
__global__ __launch_bounds__(256) void k_dipl_wsums(DiplArgs a)
{
    __shared__ double tot[2][4];
    const int tid = threadIdx.x, F = a.F;
    const int64_t s = blockIdx.x;
    const int64_t row = s / a.R;
    const int r = (int)(s - row * a.R);
    const int64_t start = a.chunk_start ? a.chunk_start[r] : (int64_t)r * F;
    const bool pair = a.pair_i != nullptr;
    const int64_t vi = pair ? a.pair_i[row] : row, vj = pair ? a.pair_j[row] : row;
    const float *wi = a.soa + (vi * 4 + 3) * a.Npad + start, *wj = a.soa + (vj * 4 + 3) * a.Npad + start;
    double s1 = 0.0, s2 = 0.0;
    for (int t = tid; t < F; t += 256) {
        const double x = (double)wi[t], y = (double)wj[t];
        s1 += pair ? x * x : x;
        s2 += y * y;
    }
    s1 = sr_wave_sum_f64(s1);
    s2 = sr_wave_sum_f64(s2);
    if ((tid & 63) == 0) {
        tot[0][tid >> 6] = s1;
        tot[1][tid >> 6] = s2;
    }
    __syncthreads();
    if (tid == 0) {
        double *o = a.wsum + s * 2;
        o[0] = (tot[0][0] + tot[0][1]) + (tot[0][2] + tot[0][3]);
        o[1] = (tot[1][0] + tot[1][1]) + (tot[1][2] + tot[1][3]);
    }
}

// ---- mode 1: the definition in float64, lag by lag from the planes --------------------------------------------------------------------
// One thread per lag (slot 0 included), frames in order: S_a - S_w / 3 with S_w from the w planes (k_ctlx_f64's shape).
__global__ __launch_bounds__(256) void k_dipl_f64(DiplArgs a)
{
    const int k = blockIdx.y * 256 + threadIdx.x, F = a.F;
    if (k > a.L) return;
    const int64_t s = blockIdx.x;
    const int64_t row = s / a.R;
    const int r = (int)(s - row * a.R);
    const int64_t start = a.chunk_start ? a.chunk_start[r] : (int64_t)r * F;
    const int64_t vi = a.pair_i ? a.pair_i[row] : row, vj = a.pair_j ? a.pair_j[row] : row;
    const float *ix = a.soa + vi * 4 * a.Npad + start, *iy = ix + a.Npad, *iz = iy + a.Npad, *iw = iz + a.Npad;
    const float *jx = a.soa + vj * 4 * a.Npad + start, *jy = jx + a.Npad, *jz = jy + a.Npad, *jw = jz + a.Npad;
    double sa = 0.0, sw = 0.0, ta = 0.0, tw = 0.0;
    for (int t = 0; t + k < F; ++t) {
        const double x = (double)ix[t] * (double)jx[t + k] + (double)iy[t] * (double)jy[t + k] + (double)iz[t] * (double)jz[t + k];
        sa += x * x;
        sw += (double)iw[t] * (double)jw[t + k];
        if (a.sym) {
            const double y = (double)jx[t] * (double)ix[t + k] + (double)jy[t] * (double)iy[t + k] + (double)jz[t] * (double)iz[t + k];
            ta += y * y;
            tw += (double)jw[t] * (double)iw[t + k];
        }
    }
    const double S = a.sym ? 0.5 * ((sa + ta) - (sw + tw) / 3.0) : sa - sw / 3.0;
    a.psum[s * a.Lp + k] = S;
}

int launch_wsums(sr_ctx *ctx, const DiplArgs &a, int64_t rows)
{
    hipLaunchKernelGGL(k_dipl_wsums, dim3((unsigned)(rows * a.R)), dim3(256), 0, ctx->stream, a);
    SR_HIP(hipGetLastError());
    return 0;
}

int launch_f64(sr_ctx *ctx, const DiplArgs &a, int64_t rows)
{
    hipLaunchKernelGGL(k_dipl_f64, dim3((unsigned)(rows * a.R), (unsigned)((a.L + 256) / 256)), dim3(256), 0, ctx->stream, a);
    SR_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int64_t sr_ct_dipolar_long_max_frames(sr_ctx *ctx)
{
    if (!ctx) return -1;
    return SR_CT_LONG_MAX_FRAMES;
}

int64_t sr_ct_dipolar_cross_long_max_frames(sr_ctx *ctx)
{
    if (!ctx) return -1;
    return SR_CT_LONG_MAX_FRAMES;
}

int sr_ct_dipolar_long_f32_dev(sr_ctx *ctx, const float *planes, int64_t Npad, int64_t nV, int64_t R, int64_t F, const int64_t *chunk_start_host,
                               int mode, double *psum_ws, double *Ct, double *dCt, double *wmean)
{
    const char *who = "sr_ct_dipolar_long_f32_dev";
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(planes && Ct && dCt && wmean, -2, "%s: null pointer", who);
    const sr_ct_rows w = {who, Npad, nV, R, F, chunk_start_host, nullptr, nullptr, 0, 0, mode, 1};
    if (int rc = sr_ct_rows_check(ctx, w, sr_ct_form_dipolar)) return rc;
    const int64_t L = F / 2, Lp = sr_ct_psum_stride(F);
    double *psum = sr_ct_psum(ctx, psum_ws, nV, R, F);
    if (!psum) return -5;
    // ---- stage the chunk starts; the chunk sums of w and w^2 live behind them ----
    sr_stage st(ctx);
    DiplArgs a;
    a.chunk_start = sr_ct_stage_tables(st, w, 2 * (size_t)(nV * R) * sizeof(double)).chunk_start;
    a.wsum = st.take<double>(2 * (size_t)(nV * R));
    if (int rc = chunk_start_host ? st.finish() : st.rc) return rc;     // tiny table: the caller's array is free again when this returns
    a.soa = planes; a.Npad = Npad; a.pair_i = a.pair_j = nullptr; a.psum = psum;
    a.R = (int)R; a.F = (int)F; a.L = (int)L; a.Lp = (int)Lp; a.sym = 0;
    if (int rc = launch_wsums(ctx, a, nV)) return rc;
    if (mode == 1) {
        if (int rc = launch_f64(ctx, a, nV)) return rc;
    } else {
        sr_ct_job job = {planes, Npad, chunk_start_host, a.chunk_start, psum, (int)R, (int)F, (int)L, (int)Lp, R * nV};
        job.planes = 4;
        job.traceless = 1;
        if (int rc = sr_launch_ct_long(ctx, job)) return rc;
    }
    if (int rc = sr_ct_finalize_weighted_f64_dev(ctx, psum, R, F, nV, Ct, dCt)) return rc;
    return sr_ct_dipolar_norm_dev(ctx, a.wsum, R, F, nV, Ct, dCt, wmean);
}

int sr_ct_dipolar_cross_long_f32_dev(sr_ctx *ctx, const float *planes, int64_t Npad, int64_t nV, int64_t R, int64_t F,
                                     const int64_t *chunk_start_host, const int32_t *pair_i_host, const int32_t *pair_j_host, int64_t nP, int sym,
                                     int mode, double *psum_ws, double *P0, double *dP0, double *Ct, double *dCt, double *wsum2)
{
    const char *who = "sr_ct_dipolar_cross_long_f32_dev";
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(planes && P0 && Ct && dCt && wsum2, -2, "%s: null pointer", who);
    const sr_ct_rows w = {who, Npad, nV, R, F, chunk_start_host, pair_i_host, pair_j_host, nP, sym, mode, 1};
    if (int rc = sr_ct_rows_check(ctx, w, sr_ct_form_dipolar_cross)) return rc;
    const int64_t L = F / 2, Lp = sr_ct_psum_stride(F);
    double *psum = sr_ct_psum(ctx, psum_ws, nP, R, F);
    if (!psum) return -5;
    // ---- the tables go up once: the chunk sums (and mode 1) read them behind the copies in stream order, and sr_launch_ct_cross_long
    // puts its slot tables in the room behind them ----
    sr_stage st(ctx);
    const sr_ct_tables t = sr_ct_stage_tables(st, w, 2 * (size_t)nP * sizeof(int32_t));
    DiplArgs a;
    a.chunk_start = t.chunk_start; a.pair_i = t.pair_i; a.pair_j = t.pair_j;
    a.soa = planes; a.Npad = Npad; a.psum = psum; a.wsum = wsum2;
    a.R = (int)R; a.F = (int)F; a.L = (int)L; a.Lp = (int)Lp; a.sym = sym;
    int err = st.rc;
    if (!err) err = launch_wsums(ctx, a, nP);
    if (!err && mode == 1) err = launch_f64(ctx, a, nP);
    if (!err && mode == 0) {
        sr_ct_pair_job job = {{planes, Npad, chunk_start_host, t.chunk_start, psum, (int)R, (int)F, (int)L, (int)Lp, R * nP},
                              nV, nP, pair_i_host, pair_j_host, t.pair_i, t.pair_j, sym, 0, &st};
        job.ct.planes = 4;
        job.ct.traceless = 1;
        if (int rc = sr_launch_ct_cross_long(ctx, job)) return rc;
    } else {                                            // no transforms follow, or a failure: the caller's arrays are free again behind finish()
        const int rc = st.finish();
        if (err || rc) return err ? err : rc;
    }
    if (int rc = sr_ct_cross_p0_dev(ctx, psum, R, F, nP, 0.0, P0, dP0)) return rc;
    if (int rc = sr_ct_finalize_weighted_f64_dev(ctx, psum, R, F, nP, Ct, dCt)) return rc;
    return sr_ct_dipolar_cross_norm_dev(ctx, wsum2, R, F, nP, Ct, dCt, P0, dP0);
}

}  // extern "C"
