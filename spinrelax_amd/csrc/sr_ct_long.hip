// sr_ct_long.hip -- kernel 1 for chunks longer than one in-LDS transform (F + L > 8192, F <= 262144): the blocked
// Wiener-Khinchin form of the Palmer-chunked P2 autocorrelation.
//
// Reference semantics: calculate_Ct_Palmer, calculate-Ct-from-traj.py:200-238, at any memory time F = int(tau / dt).
//
// The decomposition and the mean handling are those of k_ct_rfft32 (header of sr_ct32.hip): five traceless components of
// u (x) u (+ |u|^2 as a sixth signal for series that are not unit vectors), a per-(chunk, signal) constant m_c subtracted
// in float32 as d = fma(a, b, -m_c), and what the subtraction removed restored exactly in float64 from ONE scalar signal
// e[j] and its sums over the WHOLE chunk.  What changes is the transform: a chunk of F frames is cut into nb = ceil(F / B)
// blocks of B = 4096 samples (the last one zero-filled), each block is zero-padded to M = 2 B = 8192 and transformed
// (X_a, the transform length of k_ct_rfft32<16>), and for a block offset d >= 0
//     P_d(k) = sum_c w_c sum_a conj(X_a,c(k)) X_{a+d,c}(k)
// is the transform of c_d[m] = sum_a sum_j x_a[j] x_{a+d}[(j + m) mod M]: the lag sums around lag d B.  A lag
// D = d B + m (0 <= m < B) pairs frame j of block a with frame j + m of block a + d (j + m < B) or with frame j + m - B
// of block a + d + 1:   S[D] = c_d[m] + c_{d+1}[B + m].  A cyclic shift by B is a factor (-1)^k on the spectrum, so
//     Q_d(k) = P_d(k) + (-1)^k P_{d+1}(k)
// gives both pieces with ONE inverse transform per offset, of which the first B outputs are the lags d B .. d B + B - 1
// (at m = 0 the second piece is c_{d+1}[B], the one lag of the zero-padded correlation that no pair of samples reaches: zero
// in exact arithmetic, the rounding of the float32 transforms otherwise -- the error class of every other lag).
// Precision (the CPU emulation behind this design, on the ordered vectors of synth_vectors: float32 everywhere 0.4-1.2e-7,
// float64 from the cross-spectra on 1.3-2.3e-8 at every length; measured on the GPU 3e-8 on such vectors and up to 1.0e-7 of C(0)
// on tumbling and jumping ones, docs/EXPERIMENTS.md section 27): the forward transforms are float32 (where the work is: 5-6 nb per series), the sums over
// blocks, P_d, Q_d and the nd = L / B + 1 inverse transforms are float64.
//
// Launches (all on ctx->stream, in order; no atomics, every sum in a fixed order: results are bit-identical from run to
// run and for any tiling of the series):
//   k_ctl_consts   per series: the chunk means m_c, unit-vector test, K                                   (streams the planes once)
//   k_ctl_scan     per series: e[j] and its float64 suffix sums, (F - D) K + G[D] written to psum         (streams the planes once)
//   -- per tile of series (the spectra of a tile fit the workspace budget, option "ct_long_ws_mb") --
//   k_ctl_spectra  per (series, block): the float32 transforms of the 5-6 signals of a block -> HBM       (the float32 FFT work)
//   k_ctl_cross    per (series, 64 frequencies): all block spectra of the tile once -> Q_d, float64      (HBM streaming)
//   k_ctl_inverse  per (series, offset): float64 inverse real transform of Q_d, psum completed            (nd per series)
// Spectra are stored in the order the transform's threads hold them, not by frequency: entry q 256 + t (q < 8) is
// frequency k = (t >> 4) + 16 ((t & 15) + 16 q) < 2048, entry 2048 + q 256 + t is H - k, entry 4096 is k = H / 2.  The
// cross-spectra are pointwise and keep the order; the inverse transform finds k and H - k, which its first step needs together,
// 2048 entries apart.
#include "sr_ct_long.h"

namespace {

// ---- the mean terms (x 6), float64: psum[D] = (F - D) K + G[D],  G[D] = sum_{j=D}^{F-1-D} e[j];  G[0] to the constants ----
// e[j] = sum_c w_c m_c d_c[j] (+ eps_j / 3 for unit vectors), the d_c formed by the SAME float32 operations as the transforms'
// inputs (f32_sig*).  G is a suffix sum over half the series of h_i = e_i + e_{F-1-i}: tiles of 2048 from the top down, thread t
// of a tile owns eight consecutive i from the tile's top (a prefix scan over t is the suffix sum over i), a carry between tiles.
__global__ __launch_bounds__(256) void k_ctl_scan(CtlArgs a)
{
    __shared__ double hb[2048];
    __shared__ double tot[4];
    const int tid = threadIdx.x, s = blockIdx.x;
    const int v = s / a.R, r = s - v * a.R, F = a.F, L = a.L;
    const int64_t start = a.chunk_start ? a.chunk_start[r] : (int64_t)r * F;
    const float *px = a.soa + (int64_t)v * a.planes * a.Npad + start, *py = px + a.Npad, *pz = py + a.Npad;
    const CtlConst *cc = a.consts + s;
    float mm[6], wm[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        mm[c] = uniform_f(cc->m[c]);
        wm[c] = uniform_f(cc->wm[c]);
    }
    const float weps = uniform_f(cc->weps);
    const bool unit = __builtin_amdgcn_readfirstlane(cc->nsig) == 5;
    const double Kc = cc->Kc;
    double *out = a.psum + (int64_t)s * a.Lp;
    const int nh = (F + 1) / 2;                          // i = 0 .. nh - 1 (the centre frame of an odd F is its own partner)
    double carry = 0.0;
    for (int base = ((nh - 1) / 2048) * 2048; base >= 0; base -= 2048) {
#pragma unroll 2
        for (int n = 0; n < 8; ++n) {
            const int i = base + tid + 256 * n, ic = min(i, nh - 1), jc = F - 1 - ic;
            const c32 x = {px[ic], px[jc]}, y = {py[ic], py[jc]}, z = {pz[ic], pz[jc]};
            c32 acc;
            if (unit) {
                acc.x = weps * (float)fma((double)x.x, (double)x.x, fma((double)y.x, (double)y.x, fma((double)z.x, (double)z.x, -1.0)));
                acc.y = weps * (float)fma((double)x.y, (double)x.y, fma((double)y.y, (double)y.y, fma((double)z.y, (double)z.y, -1.0)));
            } else {
                acc = splat(wm[5]) * f32_sig5(x, y, z, mm[5]);
            }
            acc = pk_fma(splat(wm[0]), f32_sig0(x, y, z, mm[0]), acc);
            acc = pk_fma(splat(wm[1]), f32_sig1(x, y, mm[1]), acc);
            acc = pk_fma(splat(wm[2]), f32_sigp(x, y, mm[2]), acc);
            acc = pk_fma(splat(wm[3]), f32_sigp(x, z, mm[3]), acc);
            acc = pk_fma(splat(wm[4]), f32_sigp(y, z, mm[4]), acc);
            hb[tid + 256 * n] = i >= nh ? 0.0 : ((double)acc.x + (ic < jc ? (double)acc.y : 0.0));
        }
        __syncthreads();
        const int i0 = 8 * (255 - tid);
        double sfx[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) sfx[k] = hb[i0 + k];
#pragma unroll
        for (int k = 6; k >= 0; --k) sfx[k] += sfx[k + 1];
        const double incl = wave_scan_f64(sfx[0]);
        if ((tid & 63) == 63) tot[tid >> 6] = incl;
        __syncthreads();
        double off = incl - sfx[0];
#pragma unroll
        for (int w2 = 0; w2 < 3; ++w2) off += w2 < (tid >> 6) ? tot[w2] : 0.0;
        off += carry;
#pragma unroll
        for (int k = 0; k < 8; ++k) hb[i0 + k] = sfx[k] + off;
        carry += (tot[0] + tot[1]) + (tot[2] + tot[3]);
        __syncthreads();
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int il = tid + 256 * n, d = base + il;
            if (d < nh) out[d] = fma((double)(F - d), Kc, hb[il]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (L >= nh) out[L] = (double)(F - L) * Kc;      // even F: the window of lag L = F / 2 is empty
        a.consts[s].G0 = carry;
    }
}

// ---- cross-spectra --------------------------------------------------------------------------------------------------
// One workgroup per (series, 64 stored frequencies): per signal the nb block spectra of the tile go to LDS once, wave g forms
// P_d for d = g, g + 4, ... (float64 products of the float32 spectra, summed over the blocks in block order, then over the
// signals in signal order), the sums stay in LDS between the signals.  Weights: 6 w_c / 4 (the 4: the stored spectra are 2 X).
__global__ __launch_bounds__(256) void k_ctl_cross(CtlArgs a)
{
    extern __shared__ __align__(16) unsigned char ctl_smem[];
    const int np = a.nd + 1, nb = a.nb;
    double2 *acc = reinterpret_cast<double2 *>(ctl_smem);          // [np][64]
    c32 *X = reinterpret_cast<c32 *>(acc + (size_t)np * kKTile);   // [nb][64]
    const int tid = threadIdx.x, kk = tid & 63, dg = tid >> 6, sl = blockIdx.y;
    const int j = blockIdx.x * kKTile + kk;
    const int nsig = __builtin_amdgcn_readfirstlane(a.consts[a.s0 + sl].nsig);
    for (int i = tid; i < np * kKTile; i += 256) acc[i] = double2{0.0, 0.0};
    for (int c = 0; c < nsig; ++c) {
        __syncthreads();
        const c32 *src = a.spec + (int64_t)(sl * 6 + c) * nb * kSpecLen + blockIdx.x * kKTile;
        // (entries behind 4096 of the last tile are never written by k_ctl_spectra: they read as zero)
        for (int i = tid; i < nb * kKTile; i += 256)
            X[i] = blockIdx.x * kKTile + (i & 63) <= kH ? src[(int64_t)(i >> 6) * kSpecLen + (i & 63)] : c32{0.f, 0.f};
        __syncthreads();
        const double wq = c == 0 ? 0.25 : (c == 1 ? 0.75 : (c == 5 ? 0.5 : 3.0));
        for (int d = dg; d < np; d += 4) {
            double sr = 0.0, si = 0.0;
            for (int b = 0; b + d < nb; ++b) {
                const c32 xa = X[b * kKTile + kk], xb = X[(b + d) * kKTile + kk];
                const double ar = xa.x, ai = xa.y, br = xb.x, bi = xb.y;
                sr = fma(ai, bi, fma(ar, br, sr));                 // conj(X_a) X_{a+d}
                si = fma(-ai, br, fma(ar, bi, si));
            }
            double2 t = acc[d * kKTile + kk];
            t.x = fma(wq, sr, t.x);
            t.y = fma(wq, si, t.y);
            acc[d * kKTile + kk] = t;
        }
    }
    __syncthreads();
    if (j <= kH) {
        const double sgn = (j < kH && ((j >> 4) & 1)) ? -1.0 : 1.0;           // (-1)^k: the parity of k is that of (t >> 4)
        double2 *Q = a.Q + (int64_t)sl * a.nd * kSpecLen + j;
        for (int d = dg; d < a.nd; d += 4) {
            const double2 p0 = acc[d * kKTile + kk], p1 = acc[(d + 1) * kKTile + kk];
            Q[(int64_t)d * kSpecLen] = double2{fma(sgn, p1.x, p0.x), fma(sgn, p1.y, p0.y)};
        }
    }
}

}  // namespace

int64_t sr_ct_long_bytes_per_series(int64_t F) { return ctl_spec_bytes(F) + ctl_q_bytes(F); }

// Called by sr_ct_palmer_sums_f32_dev (sr_ct.hip) for the chunks its dispatch gives the blocked form (F + L > 8192).
int sr_launch_ct_long(sr_ctx *ctx, const sr_ct_job &j)
{
    const int F = j.F, L = j.L;
    const int64_t series = j.series;
    SR_REQUIRE(F + L > 8192 && F <= SR_CT_LONG_MAX_FRAMES, -3, "blocked C(t): F=%d outside its range", F);
    CtlArgs a;
    if (int rc = ctl_tables(ctx, &a.tab, &a.itab)) return rc;
    const int nb = (F + kB - 1) / kB, nd = L / kB + 1;
    // tiles of series whose spectra fit the budget (at least one series: 15 MB at the longest chunk)
    const int64_t per = sr_ct_long_bytes_per_series(F);
    int64_t tile = ((int64_t)ctx->ct_long_ws_mb << 20) / per;
    if (tile < 1) tile = 1;
    if (tile > series) tile = series;
    if (tile > 65535) tile = 65535;
    const size_t const_bytes = (size_t)sr_round_up(series * (int64_t)sizeof(CtlConst), 256);
    unsigned char *ws;
    if (int rc = ctl_acquire(ctx, const_bytes + (size_t)(tile * per), &ws)) return rc;

    a.soa = j.soa; a.Npad = j.Npad; a.chunk_start = j.cs_dev; a.psum = j.psum;
    a.consts = reinterpret_cast<CtlConst *>(ws);
    a.spec = reinterpret_cast<c32 *>(ws + const_bytes);
    a.Q = reinterpret_cast<double2 *>(ws + const_bytes + (size_t)tile * 6 * nb * kSpecLen * sizeof(c32));
    a.R = j.R; a.F = F; a.L = L; a.Lp = j.Lp; a.nb = nb; a.nd = nd; a.s0 = 0;
    a.planes = j.planes; a.traceless = j.traceless;
    hipLaunchKernelGGL(k_ctl_consts, dim3((unsigned)series), dim3(256), 0, ctx->stream, a);
    SR_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ctl_scan, dim3((unsigned)series), dim3(256), 0, ctx->stream, a);
    SR_HIP(hipGetLastError());
    const size_t lds_cross = (size_t)(nd + 1) * kKTile * sizeof(double2) + (size_t)nb * kKTile * sizeof(c32);
    for (int64_t s0 = 0; s0 < series; s0 += tile) {
        const unsigned ns = (unsigned)(series - s0 < tile ? series - s0 : tile);
        a.s0 = (int)s0;
        if (int rc = sr_launch(ctx, k_ctl_spectra, dim3((unsigned)nb, ns), dim3(256), ctl_spectra_lds_bytes(), a)) return rc;
        if (int rc = sr_launch(ctx, k_ctl_cross, dim3((kH + kKTile) / kKTile, ns), dim3(256), lds_cross, a)) return rc;
        if (int rc = sr_launch(ctx, k_ctl_inverse, dim3((unsigned)nd, ns), dim3(256), kCtlInverseLds, a)) return rc;
    }
    return ctl_release(ctx);
}
