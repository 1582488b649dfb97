// sr_ct_dipolar_cross.hip -- distance-weighted P2 cross-correlation between pairs of flexible spin pairs (k_ct_dipolar_cross), the
// function of dipole-dipole cross-correlated relaxation; k_ct_cross (sr_ct_cross.hip) with the r^-3 weights of k_ct_dipolar
// (sr_ct_dipolar.hip):
//     C_ij(k) = < P2(u_i(t) . u_j(t+k)) r_i(t)^-3 r_j(t+k)^-3 > / sqrt(< r_i^-6 > < r_j^-6 >)
// on the Palmer chunk table of kernel 1, from the four-plane pack a_x, a_y, a_z, w of k_pack_dipolar (per vector w = (r_ref / r)^3,
// a = u sqrt(w), so P2(u_i . u_j') w_i w_j' = 1.5 (a_i . a_j')^2 - 0.5 w_i w_j').
//
// Per (pair, chunk), the later frame from vector j as in k_ct_cross:
//     S_a(k) = sum_t (a_i(t) . a_j(t+k))^2,   S_w(k) = sum_t w_i(t) w_j(t+k),   k = 0 .. L = F/2
// (sym = 1: the mean of both directions, summed by the same lane in a fixed order, the lower vector of the pair first: (i, j) and
// (j, i) give the same bytes).  The raw sums leave as S'(k) = S_a(k) - S_w(k) / 3 in kernel 1's psum layout, row (pair, chunk), lag 0 in
// slot 0: k_ct_finalize and k_ct_cross_p0 with nothing subtracted (half = 0: 1.5 S' / (F - k) is the whole function) give the chunk
// mean of the unnormalised function, its std / (sqrt(R) - 1) and the equal-time value with its error;
// k_ct_dipolar_cross_norm scales all four by 1 / sqrt(n_i n_j), n_v the mean over the chunks of sum_t w_v^2 / F (k_ct_dipolar_norm's
// convention: a ratio of chunk means, the normaliser's own scatter is ignored; the r_ref factors cancel).  For i = j the result is
// C_dd of k_ct_dipolar with P0 = 1, to rounding.
//
// Kernels: k_ct_dipolar_cross_norm, the scaling above (its tile: dip_scale_tile, sr_ct_dipolar.h), and k_ct_dipolar_cross, on the
// scaffold of sr_ct_staged.h: one workgroup of 8 waves per (pair, chunk) (k_ct_cross's shape) stages eight series in LDS: for i and for j the three a planes
// (ct_stage_series) and the w series behind them (lds_wpos), 32 bytes per frame, 138 240 B at F = 4096: one workgroup per CU.  Per
// block of 128 lags a wave runs ct_shift_block(a_i, a_j) and dip_shift_block_w(w_i, w_j), with sym both again with the series
// exchanged; the float32 partial sums start at -min(kCenter, 8 sqrt(sum w_i^2 sum w_j^2) / F), the adaptive centre of k_ct_dipolar
// (the terms are <= w_i w_j').  Remaining lags and every lag in mode 1 take a float64 path.  While at it every wave sums w_i^2 and
// w_j^2 of the chunk in float64 and wave 0 writes them out.  No atomics, no scratch: equal input gives bit-equal output.
// A chunk must fit 32 ct_Fp(F) bytes of LDS: F <= 4896 at 160 KiB.  Longer chunks take the blocked form (sr_ct_dipolar_long.hip).
#include "sr_ct_dipolar.h"
#include "sr_ct_staged.h"
#include <cmath>

namespace {

constexpr int kDipCrossWaves = 8;

__global__ __launch_bounds__(kDipCrossWaves * 64, 2) void k_ct_dipolar_cross(CtStagedArgs a)     // soa (nV, 4, Npad); sums = wsum2 (nP, R, 2): the sum of w_i^2 and of w_j^2 over the chunk
{
    extern __shared__ __align__(16) float lds[];
    const int Fp = a.Fp, Hf = (Fp >> 3) * 12, Hw = Fp >> 1, F = a.F;
    const CtWorker w = ct_worker<kDipCrossWaves>(a, 1);
    const int tid = w.tid, lane = w.lane, wave = w.wave, p = w.row, r = w.r;
    // per vector 4 Fp floats: the three a planes (2 Hf = 3 Fp floats) and the w series behind them
    float *ai = lds, *wi = lds + 2 * Hf;
    float *aj = lds + 4 * Fp, *wj = aj + 2 * Hf;

    // sym = 1: the function of (i, j) is that of (j, i).  The pair runs with the lower vector first, so both are the same arithmetic in
    // the same order and leave the same bytes (the two directions are added into one set of sums, one after the other)
    int vi = a.pair_i[p], vj = a.pair_j[p];
    const bool swapped = a.sym && vi > vj;
    if (swapped) {
        const int t = vi;
        vi = vj;
        vj = t;
    }

    // ---- stage the eight series (coalesced dword loads; zero padding behind frame F) ----
    {
        const int64_t start = ct_chunk_start(a, w);
        const float *pi = a.soa + (int64_t)vi * 4 * a.Npad + start;
        const float *pj = a.soa + (int64_t)vj * 4 * a.Npad + start;
        const float *pwi = pi + 3 * a.Npad, *pwj = pj + 3 * a.Npad;
        ct_stage_series<kDipCrossWaves * 64>(ai, pi, pi + a.Npad, pi + 2 * a.Npad, F, Fp, Hf, tid);
        ct_stage_series<kDipCrossWaves * 64>(aj, pj, pj + a.Npad, pj + 2 * a.Npad, F, Fp, Hf, tid);
        for (int e = tid; e < Fp; e += kDipCrossWaves * 64) {
            const int q = lds_wpos(e, Hw);
            const bool in = e < F;
            wi[q] = in ? pwi[e] : 0.f;
            wj[q] = in ? pwj[e] : 0.f;
        }
    }
    __syncthreads();

    const int NW = ct_workers<kDipCrossWaves>(1), wid = ct_worker_id<kDipCrossWaves>(w);
    double *out = ct_psum_row(a, w, a.Lp);
    const int nb = ct_full_blocks(a);
    const int sym = a.sym;
    const double scale = sym ? 0.5 : 1.0;

    // ---- sum of w_i^2 and of w_j^2 over the chunk, float64, fixed order: wave 0 writes them out; every wave with a lag block takes the
    // centre of its float32 partial sums from them (k_ct_dipolar's adaptive centre: the terms of both sums are <= w_i w_j', on average
    // about sqrt(<w_i^2> <w_j^2>)) ----
    float center = kCenter;
    if (nb > 0 || wave == 0) {
        double si = 0.0, sj = 0.0;
        for (int t = lane; t < F; t += 64) {
            const int q = lds_wpos(t, Hw);
            const double x = (double)wi[q], y = (double)wj[q];
            si += x * x;
            sj += y * y;
        }
        si = wave_sum_f64(si);
        sj = wave_sum_f64(sj);
        if (wave == 0 && lane == 0) {
            double *o = a.sums + ((int64_t)p * a.R + r) * 2;
            o[swapped ? 1 : 0] = si;
            o[swapped ? 0 : 1] = sj;
        }
        center = fminf(kCenter, (float)(8.0 * sqrt(si * sj) / (double)F));
    }

    // ---- fast path: full lag blocks (lag 0 included) ----
    ct_for_each_lag_block(nb, NW, wid, lane, [=](int dw, int g, int l16) SR_CT_INLINE {
        double sa[kLagsPerLane], sw[kLagsPerLane];
        ct_zero_lags(sa);
        ct_zero_lags(sw);
        ct_shift_block(ai, aj, Hf, F, dw, g, l16, sa, center);                 // S_a of (i, j)
        dip_shift_block_w(wi, wj, Hw, F, dw, g, l16, sw, center);              // S_w of (i, j)
        if (sym) {
            ct_shift_block(aj, ai, Hf, F, dw, g, l16, sa, center);             // + (j, i)
            dip_shift_block_w(wj, wi, Hw, F, dw, g, l16, sw, center);
        }
        ct_combine_strips(sa, l16);
        ct_combine_strips(sw, l16);
        if (g == 0) {
            double *o = ct_lag_slots(out, dw, l16);
#pragma unroll
            for (int d = 0; d < kLagsPerLane; ++d) o[d] = scale * (sa[d] - sw[d] / 3.0);
        }
    });

    // ---- float64 path: remaining lags (and every lag in validation mode) ----
    ct_tail_lags<2>(nb * kLagBlock, a.L, F, NW, wid, lane, [=](int t, int d, double (&s)[2]) SR_CT_INLINE {
        const int pa = lds_pos(t, 0, Hf), pb = lds_pos(t + d, 0, Hf);
        const int wa = lds_wpos(t, Hw), wb = lds_wpos(t + d, Hw);
        const double x = ct_dot_f64(ai, aj, pa, pb);
        s[0] += x * x;
        s[1] += (double)wi[wa] * (double)wj[wb];
        if (sym) {
            const double y = ct_dot_f64(aj, ai, pa, pb);
            s[0] += y * y;
            s[1] += (double)wj[wa] * (double)wi[wb];
        }
    }, [=](int d, const double (&s)[2]) SR_CT_INLINE { out[d] = scale * (s[0] - s[1] / 3.0); });
}

// Ct, dCt (L, nP) of k_ct_finalize and P0, dP0 (nP; dP0 may be null) of k_ct_cross_p0 scaled in place by 1 / sqrt(n_i n_j), n_v the mean
// over the chunks of sum_t w_v^2 / F, the chunk sums added in chunk order.  One workgroup: 64 pairs x 64 lags; those of blockIdx.x = 0
// also scale P0 and dP0.
__global__ __launch_bounds__(256) void k_ct_dipolar_cross_norm(const double *__restrict__ wsum2, int R, int F, int L, int64_t nP,
                                                               double *__restrict__ Ct, double *__restrict__ dCt, double *__restrict__ P0,
                                                               double *__restrict__ dP0)
{
    __shared__ double inv[64];
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.y * 64;
    if (tid < 64 && p0 + tid < nP) {
        const double *s = wsum2 + (p0 + tid) * R * 2;
        double ni = 0.0, nj = 0.0;
        for (int r = 0; r < R; ++r) {
            ni += s[2 * r] / (double)F;
            nj += s[2 * r + 1] / (double)F;
        }
        inv[tid] = 1.0 / sqrt((ni / (double)R) * (nj / (double)R));
        if (blockIdx.x == 0) {
            P0[p0 + tid] *= inv[tid];
            if (dP0) dP0[p0 + tid] *= inv[tid];
        }
    }
    __syncthreads();
    dip_scale_tile(inv, L, nP, p0, Ct, dCt);
}

}  // namespace

int sr_ct_dipolar_cross_norm_dev(sr_ctx *ctx, const double *wsum2, int64_t R, int64_t F, int64_t nP, double *Ct, double *dCt, double *P0,
                                 double *dP0)
{
    const int64_t L = F / 2;
    hipLaunchKernelGGL(k_ct_dipolar_cross_norm, dim3((unsigned)((L + 63) / 64), (unsigned)((nP + 63) / 64)), dim3(256), 0, ctx->stream, wsum2,
                       (int)R, (int)F, (int)L, nP, Ct, dCt, P0, dP0);
    SR_HIP(hipGetLastError());
    return 0;
}

extern "C" {

int64_t sr_ct_dipolar_cross_max_frames(sr_ctx *ctx)
{
    if (!ctx) return -1;
    return sr_ct_lds_max_frames(sr_ct_form_dipolar_cross.bytes_per_frame, sr_lds_limit(ctx));
}

int sr_ct_dipolar_cross_f32_dev(sr_ctx *ctx, const float *planes, int64_t Npad, int64_t nV, int64_t R, int64_t F, const int64_t *chunk_start_host,
                                const int32_t *pair_i_host, const int32_t *pair_j_host, int64_t nP, int sym, int mode, double *psum_ws,
                                double *P0, double *dP0, double *Ct, double *dCt, double *wsum2)
{
    const char *who = "sr_ct_dipolar_cross_f32_dev";
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(planes && P0 && Ct && dCt && wsum2, -2, "%s: null pointer", who);
    const sr_ct_rows w = {who, Npad, nV, R, F, chunk_start_host, pair_i_host, pair_j_host, nP, sym, mode, 0};
    if (int rc = sr_ct_rows_check(ctx, w, sr_ct_form_dipolar_cross)) return rc;
    double *psum = sr_ct_psum(ctx, psum_ws, nP, R, F);
    if (!psum) return -5;
    sr_stage st(ctx);
    const sr_ct_tables t = sr_ct_stage_tables(st, w, 0);
    if (int rc = st.finish()) return rc;            // small tables: the caller's arrays are free again when this returns
    // ---- launch ----
    CtStagedArgs a = ct_staged_args(planes, Npad, t.chunk_start, psum, R, F, mode);
    a.pair_i = t.pair_i; a.pair_j = t.pair_j; a.sym = sym; a.sums = wsum2;
    if (int rc = sr_launch(ctx, k_ct_dipolar_cross, dim3((unsigned)(nP * R)), dim3(kDipCrossWaves * 64),
                           sr_ct_lds_bytes(F, sr_ct_form_dipolar_cross.bytes_per_frame), a))
        return rc;
    if (int rc = sr_ct_cross_p0_dev(ctx, psum, R, F, nP, 0.0, P0, dP0)) return rc;
    if (int rc = sr_ct_finalize_weighted_f64_dev(ctx, psum, R, F, nP, Ct, dCt)) return rc;
    return sr_ct_dipolar_cross_norm_dev(ctx, wsum2, R, F, nP, Ct, dCt, P0, dP0);
}

}  // extern "C"
