// sr_ct_dipolar.hip -- distance-weighted dipolar correlation function of a flexible spin pair (k_ct_dipolar), an extension beyond
// the reference, whose correlation functions all take the inter-spin vector as a unit vector:
//     C_dd(k) = < P2(u(t) . u(t+k)) r(t)^-3 r(t+k)^-3 > / < r^-6 >
// (Brueschweiler et al., J. Am. Chem. Soc. 114, 2289 (1992); Peter, Daura & van Gunsteren, J. Biomol. NMR 20, 297 (2001)), on the
// Palmer chunk table of kernel 1.
//
// Formulation.  Per vector, r_ref = min over the frames held of r(t), w(t) = (r_ref / r(t))^3 in (0, 1] and a(t) = u(t) sqrt(w(t)),
// so |a|^2 = w <= 1 and
//     P2(u . u') w w' = 1.5 (a . a')^2 - 0.5 w w'.
// Per (vector, chunk) two shifted-product sums: S_a(k) = sum_t (a(t) . a(t+k))^2 -- what ct_shift_block (sr_ct_shift.h) accumulates;
// every term stays in [0, 1], which its centred float32 partial sums rely on: the reason for the r_ref scaling -- and
// S_w(k) = sum_t w(t) w(t+k).
// The raw sums leave as S'(k) = S_a(k) - S_w(k) / 3 in kernel 1's psum layout, and k_ct_finalize with nothing subtracted (half = 0:
// 1.5 S' / (F - k) = [1.5 S_a - 0.5 S_w] / (F - k)) gives the chunk mean of the unnormalised function and its std / (sqrt(R) - 1);
// k_ct_dipolar_norm divides both by the chunk mean of n_r = sum_t w^2 / F.  (S' carried (F - k) / 3 once, so that the finalizer's
// 1.5 S' / (F - k) - 0.5 could stay as it was: that rounds the unnormalised function to 1e-16 ABSOLUTE, which the division by n_r turns
// into 1e-16 / <w^2> -- 3.6e-12 in float64 mode for a pair whose <w^2> is 3e-5, one close frame in 36 000.)
//
// Kernels:
//   k_dipolar_rmin   r_ref per vector: a workgroup min over the frames, no atomics
//   k_pack_dipolar   frame-major vectors (and optional distances) -> four planes per vector a_x, a_y, a_z, w in kernel 0's layout
//                    (soa[(v * 4 + c) * Npad + n], zero for n in [N, Npad)); float64 arithmetic, rounded once to float32; the tile
//                    transpose is pack_planes_tile (sr_pack_planes.h)
//   k_ct_dipolar<W>  one (vector, chunk) per workgroup or per slab of one (the scaffold and the launch ladder of sr_ct_staged.h): the three a planes staged
//                    as the direct kernel stages them, the w series behind them (parity-split 16-byte chunks, so that the 16 lag-lanes
//                    of a ds_read_b128 group read 256 consecutive bytes), 16 bytes per frame in all; per lag block ct_shift_block for
//                    S_a and the same (strip, lag-lane) partition, 8-frame window rotation and float32 partial sums of at most 16 terms
//                    for S_w (dip_shift_block_w, sr_ct_dipolar.h), both started at -8 <w^2> of the chunk instead of -kCenter; remaining lags and every
//                    lag in mode 1 by a float64 path; while staging, wave 0 of slab 0 sums w and w^2 of the chunk in float64.  No
//                    atomics, no scratch: equal input gives bit-equal output
//   k_ct_dipolar_norm  chunk means of the two sums; Ct and dCt scaled by 1 / mean n_r; <w> and <w^2> per vector
// A chunk must fit 16 ct_Fp(F) bytes of LDS: F <= 10016 at 160 KiB.  Longer chunks take the blocked form (sr_ct_dipolar_long.hip).
// Accuracy of mode 0: 2e-8 relative on C_dd was measured on wobbling pairs whose w stays within a factor 3 (C_dd >= 0.66); on mobile pairs
// whose w spans four decades (tests/test_gpu_ct_dipolar_mobile.py, docs/EXPERIMENTS.md section 38) 1.4e-7 of max(1, max |C_dd|) on C and
// 1.9e-7 / (sqrt(R) - 1) on dC, the pair form 1.1e-7 and 1.3e-7 / (sqrt(R) - 1); mode 1 1e-15.
#include "sr_ct_dipolar.h"
#include "sr_ct_staged.h"
#include "sr_pack_planes.h"
#include <cmath>

namespace {

// ------------------------------------------------------------------------------------------
// r_ref and the four-plane pack
// ------------------------------------------------------------------------------------------
constexpr int kDipVecs = kPlaneVecs;    // vectors per workgroup of k_dipolar_rmin: those of a tile of the pack, whose grid.y it is launched with
constexpr int kDipRows = 32;            // frame rows of k_dipolar_rmin

// min that keeps a NaN once it has one (a frame that is not finite must reach the host)
__device__ __forceinline__ double min_nan(double m, double r) { return (r < m || r != r) ? r : m; }

// distance of one frame: dist when given, else |v|; NaN for a frame that cannot be used (not finite, or no direction)
__device__ __forceinline__ double dip_distance(const float *__restrict__ p, const float *__restrict__ dist, int64_t di, double &len)
{
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    len = sqrt(x * x + y * y + z * z);
    double r = dist ? (double)dist[di] : len;
    if (isinf(r) || isinf(len) || len != len || (dist && !(len > 0.0))) r = NAN;
    return r;
}

__global__ __launch_bounds__(kDipVecs *kDipRows) void k_dipolar_rmin(const float *__restrict__ vecs, const float *__restrict__ dist, int64_t N,
                                                                     int64_t Vtot, int64_t v0, int64_t nV, double *__restrict__ rref)
{
    __shared__ double part[kDipRows][kDipVecs + 1];
    const int k = threadIdx.x % kDipVecs, row = threadIdx.x / kDipVecs;
    const int64_t v = (int64_t)blockIdx.x * kDipVecs + k;
    double m = INFINITY;
    if (v < nV) {
        for (int64_t f = row; f < N; f += kDipRows) {
            double len;
            m = min_nan(m, dip_distance(vecs + (f * Vtot + v0 + v) * 3, dist, f * Vtot + v0 + v, len));
        }
    }
    part[row][k] = m;
    __syncthreads();
    if (row == 0 && v < nV) {
        for (int i = 1; i < kDipRows; ++i) m = min_nan(m, part[i][k]);
        rref[v] = m;
    }
}

__global__ __launch_bounds__(256) void k_pack_dipolar(const float *__restrict__ vecs, const float *__restrict__ dist, int64_t N, int64_t Vtot,
                                                      int64_t v0, int64_t nV, const double *__restrict__ rref, float *__restrict__ soa,
                                                      int64_t Npad)
{
    pack_planes_tile<4>(vecs, N, Vtot, v0, nV, soa, Npad, [=](const float *p, int64_t di, int64_t v, float (&o)[4]) {
#pragma clang fp contract(off)
        double len;
        const double r = dip_distance(p, dist, di, len);
        const double q = rref[v] / r;
        const double w = q * q * q;
        const double s = sqrt(w) / len;
        o[0] = (float)((double)p[0] * s);
        o[1] = (float)((double)p[1] * s);
        o[2] = (float)((double)p[2] * s);
        o[3] = (float)w;
    });
}

// ------------------------------------------------------------------------------------------
// the correlation kernel
// ------------------------------------------------------------------------------------------
#ifndef SR_CT_DIP_WAVES_EU
#define SR_CT_DIP_WAVES_EU 3
#endif
template <int W>
__global__ __launch_bounds__(W * 64, SR_CT_DIP_WAVES_EU) void k_ct_dipolar(CtStagedArgs a)     // soa (nV, 4, Npad); sums (nV, R, 2): the sum of w and of w^2 over the chunk
{
    extern __shared__ __align__(16) float lds[];
    const int Fp = a.Fp, Hf = (Fp >> 3) * 12, Hw = Fp >> 1, F = a.F;
    const CtWorker w = ct_worker<W>(a, a.nslab);
    const int tid = w.tid, lane = w.lane, wave = w.wave, slab = w.slab, v = w.row, r = w.r;
    float *lw = lds + 2 * Hf;              // the w series, behind the 3 Fp floats of the a planes

    // ---- stage the four series (coalesced dword loads; zero padding behind frame F) ----
    {
        const float *px = a.soa + ((int64_t)v * 4 + 0) * a.Npad + ct_chunk_start(a, w);
        const float *py = px + a.Npad;
        const float *pz = py + a.Npad;
        const float *pw = pz + a.Npad;
        ct_stage_series<W * 64>(lds, px, py, pz, F, Fp, Hf, tid);
        for (int e = tid; e < Fp; e += W * 64) lw[lds_wpos(e, Hw)] = e < F ? pw[e] : 0.f;
    }
    __syncthreads();

    const int nb = ct_full_blocks(a);

    // ---- sum of w and of w^2 over the chunk, float64, fixed order: wave 0 of slab 0 writes them out; every wave with a lag block takes
    // the centre of its float32 partial sums from them.  The terms of both sums are about w w' <= 1, on average <w^2> of the chunk, which
    // can be far below 1: a run of 16 that starts at -8 <w^2> stays near zero, where float32 is finest (started at -kCenter it would sit
    // near -8 and round every term to 5e-7 absolute) ----
    float center = kCenter;
    if (nb > 0 || (slab == 0 && wave == 0)) {
        double s1 = 0.0, s2 = 0.0;
        for (int t = lane; t < F; t += 64) {
            const double w = (double)lw[lds_wpos(t, Hw)];
            s1 += w;
            s2 += w * w;
        }
        s1 = wave_sum_f64(s1);
        s2 = wave_sum_f64(s2);
        if (slab == 0 && wave == 0 && lane == 0) {
            double *o = a.sums + ((int64_t)v * a.R + r) * 2;
            o[0] = s1;
            o[1] = s2;
        }
        center = fminf(kCenter, (float)(8.0 * s2 / (double)F));
    }

    const int NW = ct_workers<W>(a.nslab), wid = ct_worker_id<W>(w);
    double *out = ct_psum_row(a, w, a.Lp);

    // ---- fast path: full lag blocks (lag 0 included), serpentine assignment balances the (F - lag) work ----
    ct_for_each_lag_block(nb, NW, wid, lane, [=](int dw, int g, int l16) SR_CT_INLINE {
        double sa[kLagsPerLane], sw[kLagsPerLane];
        ct_zero_lags(sa);
        ct_zero_lags(sw);
        ct_shift_block(lds, lds, Hf, F, dw, g, l16, sa, center);
        ct_combine_strips(sa, l16);
        dip_shift_block_w(lw, lw, Hw, F, dw, g, l16, sw, center);
        ct_combine_strips(sw, l16);
        if (g == 0) {
            double *o = ct_lag_slots(out, dw, l16);
#pragma unroll
            for (int d = 0; d < kLagsPerLane; ++d) o[d] = sa[d] - sw[d] / 3.0;
        }
    });

    // ---- float64 path: remaining lags (and every lag in validation mode) ----
    ct_tail_lags<2>(nb * kLagBlock, a.L, F, NW, wid, lane, [=](int j, int d, double (&s)[2]) SR_CT_INLINE {
        const double x = ct_dot_f64(lds, lds, lds_pos(j, 0, Hf), lds_pos(j + d, 0, Hf));
        s[0] += x * x;
        s[1] += (double)lw[lds_wpos(j, Hw)] * (double)lw[lds_wpos(j + d, Hw)];
    }, [=](int d, const double (&s)[2]) SR_CT_INLINE { out[d] = s[0] - s[1] / 3.0; });
}

// Ct, dCt (L, nV) of k_ct_finalize scaled in place by 1 / (mean over the chunks of n_r = sum_t w^2 / F); wmean (nV, 2) = <w>, <w^2> over
// the frames of all chunks.  One workgroup: 64 vectors x 64 lags; the chunk sums are added in chunk order.
__global__ __launch_bounds__(256) void k_ct_dipolar_norm(const double *__restrict__ wsum, int R, int F, int L, int64_t nV, double *__restrict__ Ct,
                                                         double *__restrict__ dCt, double *__restrict__ wmean)
{
    __shared__ double inv[64];
    const int tid = threadIdx.x;
    const int64_t v0 = (int64_t)blockIdx.y * 64;
    if (tid < 64 && v0 + tid < nV) {
        const double *s = wsum + (v0 + tid) * R * 2;
        double m1 = 0.0, m2 = 0.0, n = 0.0;
        for (int r = 0; r < R; ++r) {
            m1 += s[2 * r];
            m2 += s[2 * r + 1];
            n += s[2 * r + 1] / (double)F;
        }
        inv[tid] = 1.0 / (n / (double)R);
        if (blockIdx.x == 0) {
            wmean[(v0 + tid) * 2] = m1 / ((double)R * (double)F);
            wmean[(v0 + tid) * 2 + 1] = m2 / ((double)R * (double)F);
        }
    }
    __syncthreads();
    dip_scale_tile(inv, L, nV, v0, Ct, dCt);
}

}  // namespace

int sr_ct_dipolar_norm_dev(sr_ctx *ctx, const double *wsum, int64_t R, int64_t F, int64_t nV, double *Ct, double *dCt, double *wmean)
{
    const int64_t L = F / 2;
    hipLaunchKernelGGL(k_ct_dipolar_norm, dim3((unsigned)((L + 63) / 64), (unsigned)((nV + 63) / 64)), dim3(256), 0, ctx->stream, wsum, (int)R,
                       (int)F, (int)L, nV, Ct, dCt, wmean);
    SR_HIP(hipGetLastError());
    return 0;
}

extern "C" {

int64_t sr_ct_dipolar_max_frames(sr_ctx *ctx)
{
    if (!ctx) return -1;
    return sr_ct_lds_max_frames(sr_ct_form_dipolar.bytes_per_frame, sr_lds_limit(ctx));
}

int sr_pack_dipolar_f32_dev(sr_ctx *ctx, const float *vecs, const float *dist, int64_t N, int64_t Vtot, int64_t v0, int64_t nV, float *planes,
                            int64_t Npad, double *rref)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(vecs && planes && rref, -2, "sr_pack_dipolar_f32_dev: null pointer");
    dim3 grid;
    if (int rc = pack_planes_grid("sr_pack_dipolar_f32_dev", N, Vtot, v0, nV, Npad, grid)) return rc;
    hipLaunchKernelGGL(k_dipolar_rmin, dim3(grid.y), dim3(kDipVecs * kDipRows), 0, ctx->stream, vecs, dist, N, Vtot, v0, nV, rref);
    SR_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pack_dipolar, grid, dim3(256), 0, ctx->stream, vecs, dist, N, Vtot, v0, nV, rref, planes, Npad);
    SR_HIP(hipGetLastError());
    return 0;
}

int sr_ct_dipolar_f32_dev(sr_ctx *ctx, const float *planes, int64_t Npad, int64_t nV, int64_t R, int64_t F, const int64_t *chunk_start_host,
                          int mode, double *psum_ws, double *Ct, double *dCt, double *wmean)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(planes && Ct && dCt && wmean, -2, "sr_ct_dipolar_f32_dev: null pointer");
    const sr_ct_rows w = {"sr_ct_dipolar_f32_dev", Npad, nV, R, F, chunk_start_host, nullptr, nullptr, 0, 0, mode, 0};
    if (int rc = sr_ct_rows_check(ctx, w, sr_ct_form_dipolar)) return rc;
    double *psum = sr_ct_psum(ctx, psum_ws, nV, R, F);
    if (!psum) return -5;
    // ---- stage the chunk starts; the chunk sums of w and w^2 live behind them ----
    sr_stage st(ctx);
    const int64_t *cs_dev = sr_ct_stage_tables(st, w, 2 * (size_t)(nV * R) * sizeof(double)).chunk_start;
    CtStagedArgs a = ct_staged_args(planes, Npad, cs_dev, psum, R, F, mode);
    a.sums = st.take<double>(2 * (size_t)(nV * R));
    if (int rc = chunk_start_host ? st.finish() : st.rc) return rc;     // tiny table: the caller's array is free again when this returns
    if (int rc = ct_launch_slabs(ctx, k_ct_dipolar<1>, k_ct_dipolar<4>, a, R * nV, sr_ct_form_dipolar.bytes_per_frame)) return rc;
    if (int rc = sr_ct_finalize_weighted_f64_dev(ctx, psum, R, F, nV, Ct, dCt)) return rc;
    return sr_ct_dipolar_norm_dev(ctx, a.sums, R, F, nV, Ct, dCt, wmean);
}

}  // extern "C"
