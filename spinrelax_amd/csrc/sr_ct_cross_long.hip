// sr_ct_cross_long.hip -- the pair cross-correlation S_ij[k] = sum_t (u_i(t) . u_j(t+k))^2 of sr_ct_cross.hip for chunks that do not
// fit the LDS of a workgroup: the blocked transforms of sr_ct_long.hip (whose header derives the block algebra) on TWO series,
// 5462 <= F <= 262144.
//
// (u_i . u_j)^2 = T_i : T_j + |u_i|^2 |u_j|^2 / 3 with T the traceless part of u (x) u, so the lag sum of a pair is the weighted sum of
// the cross-correlations of the five (six) signals whose autocorrelations k_ctl_* form.  With x^v_a the blocks of the signals of
// series v (the subtracted constants m^v_c are the series' own: k_ctl_consts), and the later frame taken from vector j,
//     P_d(k) = sum_c w_c sum_a conj(X^i_{a,c}(k)) X^j_{a+d,c}(k),    Q_d(k) = P_d(k) + (-1)^k P_{d+1}(k),
//     S_ij[d B + m] = c_d[m] + c_{d+1}[B + m]  =  inverse transform of Q_d at m  (+ what the subtraction of the means removed).
// conj(X^i) X^j of two real signals is Hermitian: the inverse transform is k_ctl_inverse as it is.  The symmetric form (sym = 1)
// averages the cross-spectra of both directions before ONE inverse transform.
//
// The means.  With d^v_c[t] = a^v_c[t] - m^v_c the transforms' inputs (the f32_sig* operations, the same bits),
//     a^i_c[t] a^j_c[t+k] = d^i d^j + m^j_c d^i_c[t] + m^i_c d^j_c[t+k] + m^i_c m^j_c
// so lag k lacks  sum_{t < F-k} e_ij[t] + sum_{t >= k} e_ji[t] + (F - k) K_ij  with  e_ij[t] = sum_c w_c m^j_c d^i_c[t]  (e_ji: i and j
// exchanged) and K_ij = sum_c w_c m^i_c m^j_c.  With t' = F - 1 - t in the first sum both are ONE suffix sum over t' >= k of
//     h[t'] = e_ij[F - 1 - t'] + e_ji[t']            (sym = 1: the mean of this and of the same with i and j exchanged),
// taken in float64 (k_ctlx_scan).  A pair of two unit-vector series has five signals, the trace part being 1/3 + (eps_i[t] +
// eps_j[t+k]) / 3 with eps = |u|^2 - 1 below 5e-7 (its square is dropped, as in the autocorrelation): 1/3 joins K, eps / 3 joins e.
// If either series is not a unit-vector series, the pair takes |u|^2 as a sixth signal from BOTH (k_ctlx_promote tells
// k_ctl_spectra, which looks at one series, to transform it for the unit series of such a pair).
//
// Launches (all on ctx->stream, in order; no atomics, every sum in a fixed order, and nothing of a (pair, chunk) depends on what
// shares its tile: results are bit-identical from run to run and for any tiling):
//   k_ctl_consts    per series of a vector that some pair names                                           (streams those planes once)
//   k_ctlx_promote  per (pair, chunk): six signals for both series if one is not a unit-vector series
//   k_ctlx_scan     per (pair, chunk): h[t'] and its float64 suffix sums, (F - k) K + sum h -> psum; lag 0, the float64 sum of
//                   (u_i(t) . u_j(t))^2, -> slot 0 of the row                                             (streams both series twice)
//   -- per tile of pairs x chunks whose spectra and cross-spectra fit the workspace budget (option "ct_long_ws_mb") --
//   k_ctl_spectra   per (series, block), ONCE per (vector, chunk) that the tile's pairs name, however many name it
//   k_ctlx_cross    per (pair, chunk, 64 frequencies): the block spectra of both series once -> Q_d, float64
//   k_ctl_inverse   per (pair, chunk, offset): psum completed
// The distance-weighted pair form (sr_ct_dipolar_long.hip) runs the same launches on the four-plane dipolar pack with traceless = 1: five
// signals whatever |a| is (k_ctlx_promote is skipped), no eps term, no 1/3 per product, and S_a(0) - S_w(0) / 3 from the a and w planes in slot 0.
// psum has kernel 1's layout (pair, chunk, sr_ct_psum_stride(F)) with pairs in the place of vectors, so k_ct_cross_p0 and k_ct_finalize
// follow unchanged (sr_ct_cross_finish).  Mode 1 (float64 validation) is k_ctlx_f64: the definition, lag by lag from the planes.
#include <algorithm>
#include <vector>
#include "sr_ct_long.h"

namespace {

struct CtlxArgs {
    const float *soa;
    int64_t Npad;
    const int64_t *chunk_start;          // device, may be null
    const int32_t *pair_i, *pair_j;      // device, [nP]
    const int32_t *slot_i, *slot_j;      // device, [nP]: where the tile of a pair keeps the spectra of its two vectors
    CtlConst *consts;                    // [nV R] per series (k_ctl_consts)
    CtlConst *pconsts;                   // [nP R] per (pair, chunk): k_ctl_inverse reads G0 of its row there (0: the scan keeps no total back)
    double *psum;                        // (nP, R, Lp)
    const c32 *spec;                     // [tile slot][tile chunk][6][nb][kSpecLen]
    double2 *Q;                          // [tile pair][tile chunk][nd][kSpecLen]
    int64_t nPR;
    int R, F, L, Lp, nb, nd, sym;
    int p0, r0, nr;                      // the tile: its first pair, first chunk, number of chunks
    int planes;                          // planes per vector in soa: 3, or 4 for the dipolar pack (whose fourth plane is w)
    int traceless;                       // 1: five traceless signals whatever |a| is, no eps term, S_a - S_w / 3 in slot 0
};

// ---- six signals for both series of a pair if one of them is not a unit-vector series --------------------------------------------
// (weps says what k_ctl_consts found and is not written here; every write of nsig stores 6, whichever thread comes first)
__global__ __launch_bounds__(256) void k_ctlx_promote(CtlxArgs a)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.nPR) return;
    const int64_t p = s / a.R, r = s - p * a.R;
    CtlConst *ci = a.consts + (int64_t)a.pair_i[p] * a.R + r, *cj = a.consts + (int64_t)a.pair_j[p] * a.R + r;
    if (ci->weps == 0.f || cj->weps == 0.f) {
        ci->nsig = 6;
        cj->nsig = 6;
    }
}

// the transforms' inputs of two frames of one series, signal by signal
__device__ __forceinline__ void ctlx_signals(c32 x, c32 y, c32 z, const float *m, c32 *d)
{
    d[0] = f32_sig0(x, y, z, m[0]);
    d[1] = f32_sig1(x, y, m[1]);
    d[2] = f32_sigp(x, y, m[2]);
    d[3] = f32_sigp(x, z, m[3]);
    d[4] = f32_sigp(y, z, m[4]);
    d[5] = f32_sig5(x, y, z, m[5]);
}

// ---- the mean terms (x 6) and lag 0, float64 ------------------------------------------------------------------------------------------
// psum[k] = (F - k) K + sum_{t' >= k} h[t'] for k = 1 .. L, psum[0] = sum_t (u_i(t) . u_j(t))^2.  A thread forms frame t' and its mirror
// F - 1 - t' of both series as one packed pair; the suffix sum runs in tiles of 2048 from the top of the chunk down, as in k_ctl_scan.
__global__ __launch_bounds__(256) void k_ctlx_scan(CtlxArgs a)
{
    __shared__ double hb[2048];
    __shared__ double tot[4];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x;
    const int p = (int)(s / a.R), r = (int)(s - (int64_t)p * a.R), F = a.F, L = a.L;
    const int vi = a.pair_i[p], vj = a.pair_j[p];
    const int64_t start = a.chunk_start ? a.chunk_start[r] : (int64_t)r * F;
    const float *ix = a.soa + (int64_t)vi * a.planes * a.Npad + start, *iy = ix + a.Npad, *iz = iy + a.Npad;
    const float *jx = a.soa + (int64_t)vj * a.planes * a.Npad + start, *jy = jx + a.Npad, *jz = jy + a.Npad;
    const CtlConst *ci = a.consts + (int64_t)vi * a.R + r, *cj = a.consts + (int64_t)vj * a.R + r;
    float mi[6], mj[6];
    double wi[6], wj[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        mi[c] = uniform_f(ci->m[c]);
        mj[c] = uniform_f(cj->m[c]);
        wi[c] = (double)uniform_f(ci->wm[c]);
        wj[c] = (double)uniform_f(cj->wm[c]);
    }
    const bool unit = a.traceless || (uniform_f(ci->weps) != 0.f && uniform_f(cj->weps) != 0.f);
    double K6 = unit && !a.traceless ? 2.0 : 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c)
        if (c < 5 || !unit) K6 = fma(wi[c], (double)mj[c], K6);
    double *out = a.psum + s * a.Lp;
    double carry = 0.0, s0 = 0.0, sw0 = 0.0;
    for (int base = ((F - 1) / 2048) * 2048; base >= 0; base -= 2048) {
#pragma unroll 2
        for (int n = 0; n < 8; ++n) {
            const int t = base + tid + 256 * n, tc = min(t, F - 1), tm = F - 1 - tc;
            const c32 xi = {ix[tc], ix[tm]}, yi = {iy[tc], iy[tm]}, zi = {iz[tc], iz[tm]};
            const c32 xj = {jx[tc], jx[tm]}, yj = {jy[tc], jy[tm]}, zj = {jz[tc], jz[tm]};
            c32 di[6], dj[6];
            ctlx_signals(xi, yi, zi, mi, di);
            ctlx_signals(xj, yj, zj, mj, dj);
            // e_ij = sum_c 6 w_c m^j_c d^i_c and e_ji, each at t' (.x) and at its mirror (.y)
            double eij_x, eij_y, eji_x, eji_y;
            if (a.traceless) {
                eij_x = eij_y = eji_x = eji_y = 0.0;
                sw0 += t < F ? (double)iz[a.Npad + tc] * (double)jz[a.Npad + tc] : 0.0;      // the w planes
            } else if (unit) {
                eij_x = 2.0 * fma((double)xi.x, (double)xi.x, fma((double)yi.x, (double)yi.x, fma((double)zi.x, (double)zi.x, -1.0)));
                eij_y = 2.0 * fma((double)xi.y, (double)xi.y, fma((double)yi.y, (double)yi.y, fma((double)zi.y, (double)zi.y, -1.0)));
                eji_x = 2.0 * fma((double)xj.x, (double)xj.x, fma((double)yj.x, (double)yj.x, fma((double)zj.x, (double)zj.x, -1.0)));
                eji_y = 2.0 * fma((double)xj.y, (double)xj.y, fma((double)yj.y, (double)yj.y, fma((double)zj.y, (double)zj.y, -1.0)));
            } else {
                eij_x = wj[5] * (double)di[5].x;
                eij_y = wj[5] * (double)di[5].y;
                eji_x = wi[5] * (double)dj[5].x;
                eji_y = wi[5] * (double)dj[5].y;
            }
#pragma unroll
            for (int c = 0; c < 5; ++c) {
                eij_x = fma(wj[c], (double)di[c].x, eij_x);
                eij_y = fma(wj[c], (double)di[c].y, eij_y);
                eji_x = fma(wi[c], (double)dj[c].x, eji_x);
                eji_y = fma(wi[c], (double)dj[c].y, eji_y);
            }
            const double h = a.sym ? 0.5 * ((eij_x + eji_x) + (eij_y + eji_y)) : eij_y + eji_x;
            const double dot = fma((double)xi.x, (double)xj.x, fma((double)yi.x, (double)yj.x, (double)zi.x * (double)zj.x));
            hb[tid + 256 * n] = t < F ? h : 0.0;
            s0 += t < F ? dot * dot : 0.0;
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
            if (d >= 1 && d <= L) out[d] = fma((double)(F - d), K6, hb[il]);
        }
        __syncthreads();
    }
    s0 = sr_wave_sum_f64(s0);
    if ((tid & 63) == 0) tot[tid >> 6] = s0;
    __syncthreads();
    const double s0t = (tot[0] + tot[1]) + (tot[2] + tot[3]);
    if (!a.traceless) {
        if (tid == 0) {
            out[0] = s0t;
            a.pconsts[s].G0 = 0.0;
        }
        return;
    }
    // the distance-weighted pair: S_a(0) - S_w(0) / 3, the raw sum k_ct_dipolar_cross leaves in slot 0
    __syncthreads();
    sw0 = sr_wave_sum_f64(sw0);
    if ((tid & 63) == 0) tot[tid >> 6] = sw0;
    __syncthreads();
    if (tid == 0) {
        out[0] = s0t - ((tot[0] + tot[1]) + (tot[2] + tot[3])) / 3.0;
        a.pconsts[s].G0 = 0.0;
    }
}

// ---- cross-spectra of a pair ------------------------------------------------------------------------------------------------------
// One workgroup per (pair, chunk, 64 stored frequencies), the structure of k_ctl_cross with two sets of block spectra in LDS: per
// signal the nb spectra of series i and of series j, wave g forms P_d for d = g, g + 4, ... in block order, then over the signals in
// signal order; sym = 1: the j -> i sum as well, and half their sum.  Weights 6 w_c / 4 as there.
__global__ __launch_bounds__(256) void k_ctlx_cross(CtlxArgs a)
{
    extern __shared__ __align__(16) unsigned char ctlx_smem[];
    const int np = a.nd + 1, nb = a.nb;
    double2 *acc = reinterpret_cast<double2 *>(ctlx_smem);         // [np][64]
    c32 *Xi = reinterpret_cast<c32 *>(acc + (size_t)np * kKTile);  // [nb][64]
    c32 *Xj = Xi + (size_t)nb * kKTile;                            // [nb][64]
    const int tid = threadIdx.x, kk = tid & 63, dg = tid >> 6, sl = blockIdx.y;
    const int pl = sl / a.nr, rr = sl - pl * a.nr, p = a.p0 + pl, r = a.r0 + rr;
    const int j = blockIdx.x * kKTile + kk;
    const bool six = !a.traceless &&
                     (a.consts[(int64_t)a.pair_i[p] * a.R + r].weps == 0.f || a.consts[(int64_t)a.pair_j[p] * a.R + r].weps == 0.f);
    const int nsig = __builtin_amdgcn_readfirstlane(six ? 6 : 5);
    const int64_t per_sig = (int64_t)nb * kSpecLen;
    const c32 *bi = a.spec + ((int64_t)a.slot_i[p] * a.nr + rr) * 6 * per_sig + blockIdx.x * kKTile;
    const c32 *bj = a.spec + ((int64_t)a.slot_j[p] * a.nr + rr) * 6 * per_sig + blockIdx.x * kKTile;
    const double half = a.sym ? 0.5 : 1.0;
    for (int i = tid; i < np * kKTile; i += 256) acc[i] = double2{0.0, 0.0};
    for (int c = 0; c < nsig; ++c) {
        __syncthreads();
        // (entries behind 4096 of the last tile are never written by k_ctl_spectra: they read as zero)
        for (int i = tid; i < nb * kKTile; i += 256) {
            const bool in = blockIdx.x * kKTile + (i & 63) <= kH;
            const int64_t o = c * per_sig + (int64_t)(i >> 6) * kSpecLen + (i & 63);
            Xi[i] = in ? bi[o] : c32{0.f, 0.f};
            Xj[i] = in ? bj[o] : c32{0.f, 0.f};
        }
        __syncthreads();
        const double wq = half * (c == 0 ? 0.25 : (c == 1 ? 0.75 : (c == 5 ? 0.5 : 3.0)));
        for (int d = dg; d < np; d += 4) {
            double sr = 0.0, si = 0.0;
            for (int b = 0; b + d < nb; ++b) {
                const c32 xa = Xi[b * kKTile + kk], xb = Xj[(b + d) * kKTile + kk];
                const double ar = xa.x, ai = xa.y, br = xb.x, bi2 = xb.y;
                sr = fma(ai, bi2, fma(ar, br, sr));                // conj(X^i_a) X^j_{a+d}
                si = fma(-ai, br, fma(ar, bi2, si));
            }
            if (a.sym) {
                double tr = 0.0, ti = 0.0;
                for (int b = 0; b + d < nb; ++b) {
                    const c32 xa = Xj[b * kKTile + kk], xb = Xi[(b + d) * kKTile + kk];
                    const double ar = xa.x, ai = xa.y, br = xb.x, bi2 = xb.y;
                    tr = fma(ai, bi2, fma(ar, br, tr));            // conj(X^j_a) X^i_{a+d}
                    ti = fma(-ai, br, fma(ar, bi2, ti));
                }
                sr += tr;
                si += ti;
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
            const double2 q0 = acc[d * kKTile + kk], q1 = acc[(d + 1) * kKTile + kk];
            Q[(int64_t)d * kSpecLen] = double2{fma(sgn, q1.x, q0.x), fma(sgn, q1.y, q0.y)};
        }
    }
}

// ---- mode 1: the definition in float64, lag by lag from the planes ----------------------------------------------------------------------
// One thread per lag (slot 0 included), frames in order: one fixed summation order.  The on-device check of the blocked form.
__global__ __launch_bounds__(256) void k_ctlx_f64(CtlxArgs a)
{
    const int k = blockIdx.y * 256 + threadIdx.x, F = a.F;
    if (k > a.L) return;
    const int64_t s = blockIdx.x;
    const int p = (int)(s / a.R), r = (int)(s - (int64_t)p * a.R);
    const int64_t start = a.chunk_start ? a.chunk_start[r] : (int64_t)r * F;
    const float *ix = a.soa + (int64_t)a.pair_i[p] * a.planes * a.Npad + start, *iy = ix + a.Npad, *iz = iy + a.Npad;
    const float *jx = a.soa + (int64_t)a.pair_j[p] * a.planes * a.Npad + start, *jy = jx + a.Npad, *jz = jy + a.Npad;
    double sij = 0.0, sji = 0.0;
    for (int t = 0; t + k < F; ++t) {
        const double x = (double)ix[t] * (double)jx[t + k] + (double)iy[t] * (double)jy[t + k] + (double)iz[t] * (double)jz[t + k];
        sij += x * x;
        if (a.sym) {
            const double y = (double)jx[t] * (double)ix[t + k] + (double)jy[t] * (double)iy[t + k] + (double)jz[t] * (double)iz[t + k];
            sji += y * y;
        }
    }
    a.psum[s * a.Lp + k] = a.sym ? 0.5 * (sij + sji) : sij;
}

struct CtlxTile {
    int64_t p0, np;          // pairs [p0, p0 + np)
    size_t u0, nu;           // its vectors, sorted: uniq[u0 .. u0 + nu); a vector's position is its slot
};

}  // namespace

// what sr_ct_cross_f32_dev does behind its checks, for the chunks of sr_ct_rows_check(blocked = 1)
int sr_launch_ct_cross_long(sr_ctx *ctx, const sr_ct_pair_job &job)
{
    const float *soa = job.ct.soa;
    const int64_t Npad = job.ct.Npad, nV = job.nV, nP = job.nP, R = job.ct.R, F = job.ct.F, L = job.ct.L, Lp = job.ct.Lp;
    const int32_t *pair_i = job.pair_i_host, *pair_j = job.pair_j_host;
    const int planes = job.ct.planes, traceless = job.ct.traceless;
    double *psum = job.ct.psum;
    sr_stage &st = *job.st;
    const int nb = (int)((F + kB - 1) / kB), nd = (int)(L / kB + 1);
    CtlxArgs x;
    x.soa = soa; x.Npad = Npad; x.psum = psum; x.nPR = nP * R;
    x.R = (int)R; x.F = (int)F; x.L = (int)L; x.Lp = (int)Lp; x.nb = nb; x.nd = nd; x.sym = job.sym;
    x.planes = planes; x.traceless = traceless;
    x.consts = x.pconsts = nullptr; x.spec = nullptr; x.Q = nullptr; x.slot_i = x.slot_j = nullptr; x.p0 = x.r0 = 0; x.nr = (int)R;
    x.chunk_start = job.ct.cs_dev; x.pair_i = job.pair_i_dev; x.pair_j = job.pair_j_dev;
    if (job.mode == 1) {
        if (int rc = st.finish()) return rc;
        SR_REQUIRE(!traceless, -3, "blocked pair form: the traceless form has no float64 mode of its own");
        hipLaunchKernelGGL(k_ctlx_f64, dim3((unsigned)(nP * R), (unsigned)((L + 256) / 256)), dim3(256), 0, ctx->stream, x);
        SR_HIP(hipGetLastError());
        return 0;
    }

    // ---- tiles: chunks first (all R of a pair if they fit), then as many pairs as fit beside the spectra of their vectors ----
    const int64_t budget = (int64_t)ctx->ct_long_ws_mb << 20, spec_b = ctl_spec_bytes(F), q_b = ctl_q_bytes(F);
    int64_t nr = R;
    if ((2 * spec_b + q_b) * R > budget) nr = std::max<int64_t>(1, budget / (2 * spec_b + q_b));
    std::vector<int64_t> seen((size_t)nV, -1);
    std::vector<int32_t> uniq, all, slot_i((size_t)nP), slot_j((size_t)nP), slot((size_t)nV);
    std::vector<CtlxTile> tiles;
    int64_t tile_bytes = 0;
    for (int64_t p0 = 0; p0 < nP;) {
        const size_t u0 = uniq.size();
        int64_t np = 0;
        for (; p0 + np < nP; ++np) {
            const int32_t vi = pair_i[p0 + np], vj = pair_j[p0 + np];
            const int64_t add = (seen[vi] != p0) + (vj != vi && seen[vj] != p0);
            const int64_t need = ((int64_t)(uniq.size() - u0) + add) * nr * spec_b + (np + 1) * nr * q_b;
            if (np > 0 && (need > budget || (np + 1) * nr > 65535)) break;
            if (seen[vi] != p0) { seen[vi] = p0; uniq.push_back(vi); }
            if (seen[vj] != p0) { seen[vj] = p0; uniq.push_back(vj); }
        }
        std::sort(uniq.begin() + u0, uniq.end());
        for (size_t u = u0; u < uniq.size(); ++u) slot[uniq[u]] = (int32_t)(u - u0);
        for (int64_t q = p0; q < p0 + np; ++q) {
            slot_i[q] = slot[pair_i[q]];
            slot_j[q] = slot[pair_j[q]];
        }
        tiles.push_back(CtlxTile{p0, np, u0, uniq.size() - u0});
        tile_bytes = std::max(tile_bytes, (int64_t)(uniq.size() - u0) * nr * spec_b + np * nr * q_b);
        p0 += np;
    }
    all = uniq;                                      // every vector that some pair names, once
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    x.slot_i = st.put(slot_i.data(), (size_t)nP);
    x.slot_j = st.put(slot_j.data(), (size_t)nP);
    if (int rc = st.finish()) return rc;             // small tables: the host arrays are free again when this returns

    CtlArgs a;
    if (int rc = ctl_tables(ctx, &a.tab, &a.itab)) return rc;
    const size_t const_bytes = (size_t)sr_round_up(nV * R * (int64_t)sizeof(CtlConst), 256);
    const size_t pconst_bytes = (size_t)sr_round_up(nP * R * (int64_t)sizeof(CtlConst), 256);
    unsigned char *ws;
    if (int rc = ctl_acquire(ctx, const_bytes + pconst_bytes + (size_t)tile_bytes, &ws)) return rc;
    x.consts = reinterpret_cast<CtlConst *>(ws);
    x.pconsts = reinterpret_cast<CtlConst *>(ws + const_bytes);
    unsigned char *area = ws + const_bytes + pconst_bytes;
    a.soa = soa; a.Npad = Npad; a.chunk_start = x.chunk_start; a.psum = psum; a.consts = x.consts;
    a.spec = nullptr; a.Q = nullptr;
    a.R = (int)R; a.F = (int)F; a.L = (int)L; a.Lp = (int)Lp; a.nb = nb; a.nd = nd; a.s0 = 0;
    a.planes = planes; a.traceless = traceless;

    // chunk constants of the named vectors, runs of consecutive vectors in one launch (k_ctl_consts counts its series from 0)
    for (size_t u = 0; u < all.size();) {
        size_t e = u + 1;
        while (e < all.size() && all[e] == all[e - 1] + 1) ++e;
        CtlArgs c = a;
        c.soa = soa + (int64_t)all[u] * planes * Npad;
        c.consts = x.consts + (int64_t)all[u] * R;
        hipLaunchKernelGGL(k_ctl_consts, dim3((unsigned)((int64_t)(e - u) * R)), dim3(256), 0, ctx->stream, c);
        SR_HIP(hipGetLastError());
        u = e;
    }
    if (!traceless) {                                // (the traceless form has five signals whatever weps says)
        hipLaunchKernelGGL(k_ctlx_promote, dim3((unsigned)((nP * R + 255) / 256)), dim3(256), 0, ctx->stream, x);
        SR_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ctlx_scan, dim3((unsigned)(nP * R)), dim3(256), 0, ctx->stream, x);
    SR_HIP(hipGetLastError());

    const size_t lds_cross = (size_t)(nd + 1) * kKTile * sizeof(double2) + 2 * (size_t)nb * kKTile * sizeof(c32);
    for (const CtlxTile &t : tiles) {
        for (int64_t r0 = 0; r0 < R; r0 += nr) {
            const int64_t nrc = std::min(nr, R - r0);
            c32 *spec = reinterpret_cast<c32 *>(area);
            double2 *Q = reinterpret_cast<double2 *>(area + (size_t)t.nu * (size_t)nrc * (size_t)spec_b);
            // spectra: slot u holds chunks r0 .. r0 + nrc of vector uniq[u0 + u]; with all chunks in the tile the series of
            // consecutive vectors are consecutive too and go in one launch
            a.consts = x.consts; a.psum = psum;
            for (size_t u = 0; u < t.nu;) {
                size_t e = u + 1;
                if (nrc == R)
                    while (e < t.nu && uniq[t.u0 + e] == uniq[t.u0 + e - 1] + 1 && (int64_t)(e + 1 - u) * R <= 65535) ++e;
                a.s0 = (int)((int64_t)uniq[t.u0 + u] * R + r0);
                a.spec = spec + (int64_t)u * nrc * 6 * nb * kSpecLen;
                if (int rc = sr_launch(ctx, k_ctl_spectra, dim3((unsigned)nb, (unsigned)((int64_t)(e - u) * nrc)), dim3(256), ctl_spectra_lds_bytes(), a))
                    return rc;
                u = e;
            }
            x.spec = spec; x.Q = Q; x.p0 = (int)t.p0; x.r0 = (int)r0; x.nr = (int)nrc;
            if (int rc = sr_launch(ctx, k_ctlx_cross, dim3((kH + kKTile) / kKTile, (unsigned)(t.np * nrc)), dim3(256), lds_cross, x)) return rc;
            // inverse transforms: its rows are (pair, chunk) in the place of series, consecutive when the tile holds all chunks
            a.consts = x.pconsts;
            if (nrc == R) {
                a.s0 = (int)(t.p0 * R);
                a.Q = Q;
                if (int rc = sr_launch(ctx, k_ctl_inverse, dim3((unsigned)nd, (unsigned)(t.np * R)), dim3(256), kCtlInverseLds, a)) return rc;
            } else {
                for (int64_t pl = 0; pl < t.np; ++pl) {
                    a.s0 = (int)((t.p0 + pl) * R + r0);
                    a.Q = Q + pl * nrc * nd * kSpecLen;
                    if (int rc = sr_launch(ctx, k_ctl_inverse, dim3((unsigned)nd, (unsigned)nrc), dim3(256), kCtlInverseLds, a)) return rc;
                }
            }
        }
    }
    return ctl_release(ctx);
}
