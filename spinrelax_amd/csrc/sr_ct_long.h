// sr_ct_long.h -- what the two blocked forms share: sr_ct_long.hip (the autocorrelation, whose header derives the block algebra) and
// sr_ct_cross_long.hip (the same algebra on the two series of a pair).  The chunk constants, the float32 block spectra and the
// float64 inverse transform depend on one series (or one cross-spectrum) only, so both sources run the same kernels on the same
// work area (slot SR_WS_CTLONG); each source has its own cross-spectrum pass and its own restoration of the subtracted means.
// sr_ct_dipolar_long.hip runs both on the four-plane dipolar pack: CtlArgs::planes is the plane stride of a vector and
// CtlArgs::traceless asks for the five traceless signals alone (its header has the algebra); 3 and 0 are the unit-vector forms.
#pragma once
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
    int planes;                      // planes per vector in soa: 3 (unit-vector pack) or 4 (the dipolar pack a_x, a_y, a_z, w)
    int traceless;                   // 1: the five traceless signals only, whatever |a| is (sr_ct_dipolar_long.hip)
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
    const float *px = a.soa + (int64_t)v * a.planes * a.Npad + start, *py = px + a.Npad, *pz = py + a.Npad;
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
        // traceless: five signals as for unit vectors, but neither the constant 1/3 per product nor the eps term (weps = 0): the
        // caller's function has no trace part (sr_ct_dipolar_long.hip)
        const bool unit = a.traceless || fmaxf(fmaxf(red[0][6], red[1][6]), fmaxf(red[2][6], red[3][6])) < kUnitTolF;
        CtlConst c;
        double Kc = unit && !a.traceless ? 2.0 : 0.0;          // 6 x the 1/3 per product of unit vectors; the traceless form has none
        for (int i = 0; i < 6; ++i) {
            const float mean = ((red[0][i] + red[1][i]) + (red[2][i] + red[3][i])) * invF;
            c.m[i] = __builtin_bit_cast(float, __builtin_bit_cast(int, mean) & (int)0xFFFFFFF0);
            c.wm[i] = wgt[i] * c.m[i];
            if (i < 5 || !unit) Kc = fma((double)wgt[i] * (double)c.m[i], (double)c.m[i], Kc);
        }
        c.weps = unit && !a.traceless ? 2.0f : 0.f;
        c.nsig = unit ? 5 : 6;
        c.Kc = Kc;
        c.G0 = 0.0;
        a.consts[s] = c;
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
    const float *px = a.soa + (int64_t)v * a.planes * a.Npad + start;
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

// ---- host side -------------------------------------------------------------------------------------------------------
// bytes of work area per series: its 6 nb block spectra; per cross-spectrum set: nd spectra in float64
inline int64_t ctl_spec_bytes(int64_t F) { return 6 * ((F + kB - 1) / kB) * kSpecLen * (int64_t)sizeof(c32); }
inline int64_t ctl_q_bytes(int64_t F) { return ((F / 2) / kB + 1) * kSpecLen * (int64_t)sizeof(double2); }

// the tables of both transforms, created on first use
inline int ctl_tables(sr_ctx *ctx, const Ct32Tab **tab32, const double2 **itab_out)
{
    const Ct32Tab *t = (const Ct32Tab *)sr_ct32_tables(ctx);
    if (!t) return -5;
    double2 *itab = (double2 *)sr_workspace(ctx, SR_WS_CTLONG_TAB, (size_t)kH * sizeof(double2));
    if (!itab) return -5;
    if (!ctx->ctlong_table_ready) {
        hipLaunchKernelGGL(k_ctl_init_table, dim3(kH / 256), dim3(256), 0, ctx->stream, itab);
        SR_HIP(hipGetLastError());
        SR_HIP(hipStreamSynchronize(ctx->stream));      // once per context: later launches may come on other streams
        ctx->ctlong_table_ready = 1;
    }
    *tab32 = t + f32_tab_set(16);
    *itab_out = itab;
    return 0;
}

// One context is driven from several streams (spinrelax_amd/pipeline.py alternates the C(t) launches of successive batches
// between two): the work area is one per context, so a call first waits for the previous blocked call's last kernel (ctl_acquire,
// before its first launch) and leaves an event behind its own (ctl_release).
inline int ctl_acquire(sr_ctx *ctx, size_t bytes, unsigned char **ws)
{
    if (!ctx->ctlong_ev) SR_HIP(hipEventCreateWithFlags(&ctx->ctlong_ev, hipEventDisableTiming));
    *ws = (unsigned char *)sr_workspace(ctx, SR_WS_CTLONG, bytes);
    if (!*ws) return -5;
    if (ctx->ctlong_ev_set) SR_HIP(hipStreamWaitEvent(ctx->stream, ctx->ctlong_ev, 0));
    return 0;
}
inline int ctl_release(sr_ctx *ctx)
{
    SR_HIP(hipEventRecord(ctx->ctlong_ev, ctx->stream));
    ctx->ctlong_ev_set = 1;
    return 0;
}

constexpr size_t kCtlInverseLds = (size_t)kH * sizeof(double2);
static_assert(ctl_spectra_lds_bytes() <= 64 * 1024, "k_ctl_spectra: the image is meant to fit the default LDS grant");

}  // namespace
