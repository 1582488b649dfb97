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
// Precision (the CPU emulation behind this design: float32 everywhere 0.4-1.2e-7, float64 from the cross-spectra on
// 1.3-2.3e-8 at every length): the forward transforms are float32 (where the work is: 5-6 nb per series), the sums over
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
#include "sr_internal.h"
#include "sr_ct32_fft.h"

namespace {

constexpr int kB = 4096;             // samples per block
constexpr int kH = 4096;             // complex points of a block's real-input transform (M = 8192)
constexpr int kSpecLen = 4160;       // entries reserved per stored spectrum (4097 used; a multiple of 64)
constexpr int kKTile = 64;           // frequencies per workgroup of the cross-spectrum pass

struct CtlConst {                    // per series
    float m[6];                      // m_c
    float wm[6];                     // 6 w_c m_c
    float weps;                      // weight of eps = |u|^2 - 1 in e[j] (2 for unit vectors)
    int nsig;                        // 5 (unit vectors) or 6
    double Kc;                       // 6 (sum_c w_c m_c^2 (+ 1/3))
    double G0;                       // sum of e over the chunk (x 6)
};

struct CtlArgs {
    const float *soa;
    int64_t Npad;
    const int64_t *chunk_start;      // device, may be null
    CtlConst *consts;                // [series]
    double *psum;                    // (nV, R, Lp)
    const Ct32Tab *tab;              // float32 tables of the 8192-point transform
    c32 *spec;                       // [tile series][6][nb][kSpecLen]
    double2 *Q;                      // [tile series][nd][kSpecLen]
    const double2 *itab;             // exp(+2 pi i e / 8192), e < 4096
    int R, F, L, Lp, nb, nd;
    int s0;                          // first series of the tile
};

__device__ __forceinline__ float uniform_f(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// ---- chunk constants ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ctl_consts(CtlArgs a)
{
    __shared__ float red[4][8];
    const int tid = threadIdx.x, s = blockIdx.x;
    const int v = s / a.R, r = s - v * a.R, F = a.F;
    const int64_t start = a.chunk_start ? a.chunk_start[r] : (int64_t)r * F;
    const float *px = a.soa + (int64_t)v * 3 * a.Npad + start, *py = px + a.Npad, *pz = py + a.Npad;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f, s5 = 0.f, emax = 0.f;
    for (int j = tid; j < F; j += 256) {
        const float x = px[j], y = py[j], z = pz[j];
        const float xx = x * x, yy = y * y, zz = z * z, q = xx + yy;
        s0 += (zz + zz) - q;
        s1 += xx - yy;
        s2 = fmaf(x, y, s2);
        s3 = fmaf(x, z, s3);
        s4 = fmaf(y, z, s4);
        s5 += q + zz;
        emax = fmaxf(emax, fabsf((q + zz) - 1.0f));
    }
    s0 = wave_total_f32(s0); s1 = wave_total_f32(s1); s2 = wave_total_f32(s2);
    s3 = wave_total_f32(s3); s4 = wave_total_f32(s4); s5 = wave_total_f32(s5);
    emax = wave_max_f32(emax);
    if ((tid & 63) == 63) {
        float *o = red[tid >> 6];
        o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3; o[4] = s4; o[5] = s5; o[6] = emax;
    }
    __syncthreads();
    if (tid == 0) {
        // m_c: the chunk mean with its low four mantissa bits cleared, as in k_ct_rfft32 (3 m_c and 12 m_c exact in float32)
        const float wgt[6] = {1.0f, 3.0f, 12.0f, 12.0f, 12.0f, 2.0f};
        const float invF = 1.0f / (float)F;
        const bool unit = fmaxf(fmaxf(red[0][6], red[1][6]), fmaxf(red[2][6], red[3][6])) < kUnitTolF;
        CtlConst c;
        double Kc = unit ? 2.0 : 0.0;
        for (int i = 0; i < 6; ++i) {
            const float mean = ((red[0][i] + red[1][i]) + (red[2][i] + red[3][i])) * invF;
            c.m[i] = __builtin_bit_cast(float, __builtin_bit_cast(int, mean) & (int)0xFFFFFFF0);
            c.wm[i] = wgt[i] * c.m[i];
            if (i < 5 || !unit) Kc = fma((double)wgt[i] * (double)c.m[i], (double)c.m[i], Kc);
        }
        c.weps = unit ? 2.0f : 0.f;
        c.nsig = unit ? 5 : 6;
        c.Kc = Kc;
        c.G0 = 0.0;
        a.consts[s] = c;
    }
}

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
    const float *px = a.soa + (int64_t)v * 3 * a.Npad + start, *py = px + a.Npad, *pz = py + a.Npad;
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

// ---- block spectra --------------------------------------------------------------------------------------------------
// the block's samples of one plane through a buffer resource that covers exactly the block's frames of the chunk: frames past
// the chunk read as 0
__device__ __forceinline__ void ctl_load(c32 *dst, const float *plane, int Fb, bool even, int tid)
{
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(plane), (short)0, Fb * 4, 0x00020000);
    if (even) {
#pragma unroll
        for (int n1 = 0; n1 < 8; ++n1)
            dst[n1] = __builtin_bit_cast(c32, __builtin_amdgcn_raw_buffer_load_b64(rs, 8 * (tid + 256 * n1), 0, 0));
    } else {
#pragma unroll
        for (int n1 = 0; n1 < 8; ++n1) {
            const int ob = 8 * (tid + 256 * n1);
            dst[n1] = c32{__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, ob, 0, 0)),
                          __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, ob + 4, 0, 0))};
        }
    }
}

constexpr size_t ctl_spectra_lds_bytes() { return (size_t)(rfft_img_slots(16) + 256 + 1024 + 256) * sizeof(c32); }

__global__ __launch_bounds__(256, 3) void k_ctl_spectra(CtlArgs a)
{
    extern __shared__ __align__(16) unsigned char ctl_smem[];
    c32 *lds = reinterpret_cast<c32 *>(ctl_smem);
    constexpr int N1 = 16, NZ = 8;                                 // a block fills the first NZ of the N1 inputs of a thread
    c32 *tw1 = lds + rfft_img_slots(N1) + 256;
    c32 *tw3 = tw1 + 1024;
    const int tid0 = threadIdx.x, blk = blockIdx.x, sl = blockIdx.y, s = a.s0 + sl;
    const int v = s / a.R, r = s - v * a.R;
    const int64_t start = (a.chunk_start ? a.chunk_start[r] : (int64_t)r * a.F) + (int64_t)blk * kB;
    const int Fb = min(kB, a.F - blk * kB);                        // frames of the chunk in this block (>= 1)
    const float *px = a.soa + (int64_t)v * 3 * a.Npad + start;
    const bool even = ((start | a.Npad | (int64_t)Fb) & 1) == 0;   // frames 2m, 2m + 1 of every plane share an aligned 8 bytes
    {
        const int j = ((tid0 & 15) * (tid0 >> 4)) & 255;
        lds[rfft_img_slots(N1) + tid0] = c32{a.tab->w2[2 * j], a.tab->w2[2 * j + 1]};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) tw1[256 * jj + tid0] = c32{a.tab->w1[jj][2 * tid0], a.tab->w1[jj][2 * tid0 + 1]};
        tw3[tid0] = c32{a.tab->w3[2 * tid0], a.tab->w3[2 * tid0 + 1]};
    }
    const CtlConst *cc = a.consts + s;
    const int nsig = __builtin_amdgcn_readfirstlane(cc->nsig);
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < nsig; ++c) {
        asm volatile("" ::: "memory");
        const int tid = opaque(tid0);
        const float mc = uniform_f(cc->m[c]);
        c32 sig[N1];
        {
            c32 ar[NZ], br[NZ];
            ctl_load(ar, px + (int64_t)__builtin_amdgcn_readfirstlane(f32_plane_a(c)) * a.Npad, Fb, even, tid);
            ctl_load(br, px + (int64_t)__builtin_amdgcn_readfirstlane(f32_plane_b(c)) * a.Npad, Fb, even, tid);
            if (c == 0 || c == 5) {
                c32 zr[NZ];
                ctl_load(zr, px + 2 * a.Npad, Fb, even, tid);
#pragma unroll
                for (int n1 = 0; n1 < NZ; ++n1) ar[n1] = c == 0 ? f32_sig0(ar[n1], br[n1], zr[n1], mc) : f32_sig5(ar[n1], br[n1], zr[n1], mc);
            } else if (c == 1) {
#pragma unroll
                for (int n1 = 0; n1 < NZ; ++n1) ar[n1] = f32_sig1(ar[n1], br[n1], mc);
            } else {
#pragma unroll
                for (int n1 = 0; n1 < NZ; ++n1) ar[n1] = f32_sigp(ar[n1], br[n1], mc);
            }
            // frames behind the chunk hold 0 in every signal (they are part of the zero padding)
#pragma unroll
            for (int n1 = 0; n1 < NZ; ++n1) {
                c32 d = ar[n1];
                d.x = 2 * (tid + 256 * n1) < Fb ? d.x : 0.f;
                d.y = 2 * (tid + 256 * n1) + 1 < Fb ? d.y : 0.f;
                sig[n1] = d;
            }
#pragma unroll
            for (int n1 = NZ; n1 < N1; ++n1) sig[n1] = c32{0.f, 0.f};
        }
        c32 w[16];
        rfft32_workgroup<N1, true>(sig, w, lds, tw1, tid);
        __syncthreads();
        // 2 X[k] = S - i T and 2 conj X[H - k] = S + i T with S = Z[k] + conj Z[H-k], T = w_M^k (Z[k] - conj Z[H-k]) (see k_ct_rfft32);
        // the factor 2 stays in the stored spectra and leaves with the weights of the cross-spectra
        const int k1 = (tid >> 4) & 15, k2a = tid & 15;
        const int pt = k1 != 0 ? (N1 - k1) * 16 + (15 - k2a) : (k2a != 0 ? 16 - k2a : 0);
        const int off0 = tid == 0 ? 1 : 0;
        const c32 *b = lds + 17 * pt + off0;
        const c32 wb = tw3[k1 + N1 * k2a];
        c32 *out = a.spec + ((int64_t)(sl * 6 + c) * a.nb + blk) * kSpecLen + tid;
#pragma unroll
        for (int q = 0; q < 8; q += 2) {
            const c32 zk0 = w[bitrev<4>(q)], zm0 = b[15 - q], zk1 = w[bitrev<4>(q + 1)], zm1 = b[14 - q];
            const c32 S0 = add_conj(zk0, zm0), S1 = add_conj(zk1, zm1);
            c32 T0 = sub_conj(zk0, zm0), T1 = sub_conj(zk1, zm1);
            cmulf2(T0, mulf_w32_rt(wb, q), T1, mulf_w32_rt(wb, q + 1));
            const c32 A0 = pair_re(S0, T0), B0 = pair_im(S0, T0), A1 = pair_re(S1, T1), B1 = pair_im(S1, T1);
            out[256 * q] = c32{A0.x, B0.x};
            out[2048 + 256 * q] = c32{A0.y, -B0.y};
            out[256 * (q + 1)] = c32{A1.x, B1.x};
            out[2048 + 256 * (q + 1)] = c32{A1.y, -B1.y};
        }
        if (off0) {                                                // k = H/2 (k2b = 8) mirrors onto itself
            const c32 zk = w[bitrev<4>(8)];
            const c32 D = {0.0f, 2.0f * zk.y};
            const c32 T = cmulf(D, mulf_w32_rt(wb, 8));
            out[4096] = c32{2.0f * zk.x + T.y, -T.x};
        }
        __syncthreads();
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

// ---- inverse transforms ---------------------------------------------------------------------------------------------
__global__ void k_ctl_init_table(double2 *tab)               // exp(+2 pi i e / 8192), e < 4096
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    double sn, cs;
    sincospi((double)e / 4096.0, &sn, &cs);
    tab[e] = double2{cs, sn};
}

__device__ __forceinline__ double2 cmul64(double2 a, double2 b) { return double2{fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x)}; }

// One workgroup per (series, offset d): Y[k] = (Q[k] + conj Q[H-k]) + i conj(w_M^k) (Q[k] - conj Q[H-k]), the inverse complex
// transform of Y (radix 2, decimation in frequency: eight steps through LDS, the last four in registers on 16 consecutive
// points) is y[n] = M (c[2n] + i c[2n + 1]); lags d B + m, m < B, are completed in psum: (c[m] + mean terms) / 6.
__global__ __launch_bounds__(256) void k_ctl_inverse(CtlArgs a)
{
    extern __shared__ __align__(16) unsigned char ctl_smem[];
    double2 *lds = reinterpret_cast<double2 *>(ctl_smem);          // kH points
    const int tid = threadIdx.x, d = blockIdx.x, sl = blockIdx.y, s = a.s0 + sl;
    const double2 *Q = a.Q + ((int64_t)sl * a.nd + d) * kSpecLen;
    const double2 *T = a.itab;
#pragma unroll 2
    for (int q = 0; q < 8; ++q) {
        const int k = (tid >> 4) + 16 * ((tid & 15) + 16 * q);
        const double2 P = Q[256 * q + tid], Pm = Q[2048 + 256 * q + tid];     // Q[k], Q[H - k]
        const double2 S = {P.x + Pm.x, P.y - Pm.y}, D = {P.x - Pm.x, P.y + Pm.y};
        const double2 td = cmul64(T[k], D);
        const double2 U = {-td.y, td.x};
        lds[k] = double2{S.x + U.x, S.y + U.y};
        if (k != 0) lds[kH - k] = double2{S.x - U.x, -(S.y - U.y)};
    }
    if (tid == 0) {
        const double2 P = Q[4096];                                 // k = H/2 is its own partner
        lds[kH / 2] = double2{2.0 * P.x, -2.0 * P.y};
    }
    for (int st = 0; st < 8; ++st) {
        __syncthreads();
        const int lh = 11 - st, half = 1 << lh;
#pragma unroll 2
        for (int n = 0; n < 8; ++n) {
            const int bf = tid + 256 * n, jj = bf & (half - 1), i0 = ((bf >> lh) << (lh + 1)) + jj, i1 = i0 + half;
            const double2 A = lds[i0], Bv = lds[i1];
            lds[i0] = double2{A.x + Bv.x, A.y + Bv.y};
            lds[i1] = cmul64(double2{A.x - Bv.x, A.y - Bv.y}, T[(jj << st) << 1]);
        }
    }
    __syncthreads();
    double2 u[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) u[p] = lds[16 * tid + p];
    {
        constexpr double cs16[8] = {1.0, 0.9238795325112867, 0.7071067811865476, 0.3826834323650898, 0.0,
                                    -0.3826834323650898, -0.7071067811865476, -0.9238795325112867};
        constexpr double sn16[8] = {0.0, 0.3826834323650898, 0.7071067811865476, 0.9238795325112867, 1.0,
                                    0.9238795325112867, 0.7071067811865476, 0.3826834323650898};
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const int half = 8 >> st;
#pragma unroll
            for (int bf = 0; bf < 8; ++bf) {
                const int jj = bf & (half - 1), i0 = ((bf / half) * 2 * half) + jj, i1 = i0 + half, e = jj << st;
                const double2 A = u[i0], Bv = u[i1];
                u[i0] = double2{A.x + Bv.x, A.y + Bv.y};
                u[i1] = cmul64(double2{A.x - Bv.x, A.y - Bv.y}, double2{cs16[e], sn16[e]});
            }
        }
    }
    __syncthreads();                                               // every thread has its points: the image now takes the lags
    double *lag = reinterpret_cast<double *>(ctl_smem);
    {
        // u[p] = y[rev12(16 tid + p)] = y[256 rev4(p) + rev8(tid)]; n < 2048 (lags below B) are the even p
        const int n0 = (int)(__builtin_bitreverse32((unsigned)tid) >> 24);
#pragma unroll
        for (int p = 0; p < 16; p += 2) {
            const int n = 256 * bitrev<4>(p) + n0;
            lag[2 * n] = u[p].x;
            lag[2 * n + 1] = u[p].y;
        }
    }
    __syncthreads();
    double *out = a.psum + (int64_t)s * a.Lp;
    const double G0 = a.consts[s].G0, inv = 1.0 / 8192.0, sixth = 1.0 / 6.0;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int m = tid + 256 * i, D = d * kB + m;
        if (D >= 1 && D <= a.L) out[D] = fma(lag[m], inv, out[D] + G0) * sixth;
    }
}

}  // namespace

int64_t sr_ct_long_bytes_per_series(int64_t F)
{
    const int64_t nb = (F + kB - 1) / kB, nd = (F / 2) / kB + 1;
    return 6 * nb * kSpecLen * (int64_t)sizeof(c32) + nd * kSpecLen * (int64_t)sizeof(double2);
}

// Called by sr_ct_palmer_sums_f32_dev (sr_ct.hip) for the chunks its dispatch gives the blocked form (F + L > 8192).
int sr_launch_ct_long(sr_ctx *ctx, const sr_ct_job &j)
{
    const int F = j.F, L = j.L;
    const int64_t series = j.series;
    SR_REQUIRE(F + L > 8192 && F <= SR_CT_LONG_MAX_FRAMES, -3, "blocked C(t): F=%d outside its range", F);
    const Ct32Tab *tab32 = (const Ct32Tab *)sr_ct32_tables(ctx);
    if (!tab32) return -5;
    double2 *itab = (double2 *)sr_workspace(ctx, SR_WS_CTLONG_TAB, (size_t)kH * sizeof(double2));
    if (!itab) return -5;
    if (!ctx->ctlong_table_ready) {
        hipLaunchKernelGGL(k_ctl_init_table, dim3(kH / 256), dim3(256), 0, ctx->stream, itab);
        SR_HIP(hipGetLastError());
        SR_HIP(hipStreamSynchronize(ctx->stream));      // once per context: later launches may come on other streams
        ctx->ctlong_table_ready = 1;
    }
    const int nb = (F + kB - 1) / kB, nd = L / kB + 1;
    // tiles of series whose spectra fit the budget (at least one series: 15 MB at the longest chunk)
    const int64_t per = sr_ct_long_bytes_per_series(F);
    int64_t tile = ((int64_t)ctx->ct_long_ws_mb << 20) / per;
    if (tile < 1) tile = 1;
    if (tile > series) tile = series;
    if (tile > 65535) tile = 65535;
    const size_t const_bytes = (size_t)sr_round_up(series * (int64_t)sizeof(CtlConst), 256);
    // One context is driven from several streams (spinrelax_amd/pipeline.py alternates the C(t) launches of successive batches
    // between two): the work area is one per context, so a call first waits for the previous call's last kernel.
    if (!ctx->ctlong_ev) SR_HIP(hipEventCreateWithFlags(&ctx->ctlong_ev, hipEventDisableTiming));
    unsigned char *ws = (unsigned char *)sr_workspace(ctx, SR_WS_CTLONG, const_bytes + (size_t)(tile * per));
    if (!ws) return -5;
    if (ctx->ctlong_ev_set) SR_HIP(hipStreamWaitEvent(ctx->stream, ctx->ctlong_ev, 0));

    CtlArgs a;
    a.soa = j.soa; a.Npad = j.Npad; a.chunk_start = j.cs_dev; a.psum = j.psum; a.tab = tab32 + f32_tab_set(16); a.itab = itab;
    a.consts = reinterpret_cast<CtlConst *>(ws);
    a.spec = reinterpret_cast<c32 *>(ws + const_bytes);
    a.Q = reinterpret_cast<double2 *>(ws + const_bytes + (size_t)tile * 6 * nb * kSpecLen * sizeof(c32));
    a.R = j.R; a.F = F; a.L = L; a.Lp = j.Lp; a.nb = nb; a.nd = nd; a.s0 = 0;
    hipLaunchKernelGGL(k_ctl_consts, dim3((unsigned)series), dim3(256), 0, ctx->stream, a);
    SR_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ctl_scan, dim3((unsigned)series), dim3(256), 0, ctx->stream, a);
    SR_HIP(hipGetLastError());
    const size_t lds_cross = (size_t)(nd + 1) * kKTile * sizeof(double2) + (size_t)nb * kKTile * sizeof(c32);
    const size_t lds_inv = (size_t)kH * sizeof(double2);
    static_assert(ctl_spectra_lds_bytes() <= 64 * 1024, "k_ctl_spectra: the image is meant to fit the default LDS grant");
    for (int64_t s0 = 0; s0 < series; s0 += tile) {
        const unsigned ns = (unsigned)(series - s0 < tile ? series - s0 : tile);
        a.s0 = (int)s0;
        if (int rc = sr_launch(ctx, k_ctl_spectra, dim3((unsigned)nb, ns), dim3(256), ctl_spectra_lds_bytes(), a)) return rc;
        if (int rc = sr_launch(ctx, k_ctl_cross, dim3((kH + kKTile) / kKTile, ns), dim3(256), lds_cross, a)) return rc;
        if (int rc = sr_launch(ctx, k_ctl_inverse, dim3((unsigned)nd, ns), dim3(256), lds_inv, a)) return rc;
    }
    SR_HIP(hipEventRecord(ctx->ctlong_ev, ctx->stream));
    ctx->ctlong_ev_set = 1;
    return 0;
}
