// sr_ct_fft64.hip -- kernel 1 with complex float64 transforms (k_ct_fft): the Wiener-Khinchin form of the Palmer-chunked P2
// autocorrelation, one workgroup per (chunk, vector) series with the whole transform of M = 2048 / 4096 / 6144 / 8192 points in
// LDS, accurate to 1e-15; and the twiddle table it shares with the real-input kernel (sr_ct_rfft64.hip).  Which chunks take it
// (option "ct_fft"): the dispatch of sr_ct.hip.  The float32 counterpart is sr_ct32.hip.
//
// Reference semantics: calculate_Ct_Palmer, calculate-Ct-from-traj.py:200-238 (see include/spinrelax_hip.h).
#include "sr_fft64.h"

namespace {

// S[lag] = sum_j (u(j).u(j+lag))^2 is the sum of six ordinary autocorrelations: with
//   a = (x^2, y^2, z^2, xy, xz, yz),  (u.u')^2 = a1 a1' + a2 a2' + a3 a3' + 2 (a4 a4' + a5 a5' + a6 a6'),
// so S = IFFT( sum_c w_c |FFT(a_c)|^2 ) on the chunk zero-padded to M >= F + L points (Wiener-Khinchin).  In float64
// this is ~13x fewer operations than the 4 F L / 2 FMAs of the direct kernel at F = 4096, and more accurate (1e-14
// instead of the float32 dot products' 1e-8).  What makes it a one-workgroup-per-series kernel is the 160 KB of LDS:
// a complete 8192-point complex float64 transform (128 KB + padding) stays on the CU.
//
// One workgroup of 256 threads owns one (chunk, vector) series.  M = N1 * 256, N1 = 8, 16 or 32; four-step
// decomposition N1 x 32 x 8 with every small transform in registers:
//   1. thread n2 holds the N1 samples n = n2 + 256 n1, transforms them (radix-2 DIF, constant twiddles), applies
//      the twiddle w_M^(n2 k1);
//   2. exchange through LDS; thread (k1, n2 mod 8) transforms 32 samples n2 = lo + 8 h, twiddle w_256^(lo k2a);
//   3. exchange; thread q transforms the 8 samples of group g = k1 + N1 k2a: X[g + 32 N1 k2b].
// Real signals are transformed in pairs (p + i q); the power spectra come out of Z(k) and conj Z(M-k), exchanged
// through LDS once more.  The weighted power spectrum (real, even) then runs through the same transform; its real
// part / M is S[lag], written where the direct kernel writes (raw sums per chunk; k_ct_finalize is shared).
// LDS addresses are padded (one slot per 8, eight per 256) so that all three access patterns are conflict-free.

__global__ void k_fft_init_table(double *tab)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    double sn, cs;
    if (t < 1280) {
        if (t < 1024) sincospi((double)t / 4096.0, &sn, &cs);
        else sincospi((double)(t - 1024) / 3072.0, &sn, &cs);
    } else if (t < 1280 + 2 * 768) {
        const int u = t - 1280, set = u / 768, j = u - set * 768, which = j >> 8, i = j & 255;
        const double H = set == 0 ? 3072.0 : 4096.0;
        const double len = which == 0 ? H : (which == 1 ? 256.0 : 2.0 * H);
        sincospi(2.0 * (double)i / len, &sn, &cs);
    } else {
        return;
    }
    tab[2 * t] = cs;
    tab[2 * t + 1] = -sn;
}

struct CtFftArgs {
    const float *soa;
    int64_t Npad;
    const int64_t *chunk_start;   // device, may be null
    const Ct64Tab *tab;
    double *psum;                 // (nV, R, Lp)
    int R, F, L, Lp;
};

// HALF: the chunk fills at most 256 NZ samples (NZ = N1/2, or 16 of 24: the F = 4096 case): the thread's samples
// beyond NZ are known to be zero and are not loaded
template <int N1, bool HALF>
__global__ __launch_bounds__(256) void k_ct_fft(CtFftArgs a)
{
    extern __shared__ __align__(16) unsigned char fft_smem[];
    cplx *lds = reinterpret_cast<cplx *>(fft_smem);
    constexpr int M = N1 * 256;
    constexpr int G = N1 / 8;
    constexpr int NZ = HALF ? (N1 == 24 ? 16 : N1 / 2) : N1;
    const int tid = threadIdx.x;
    const int v = blockIdx.x / a.R, r = blockIdx.x - v * a.R;
    const int F = a.F;
    const int64_t start = a.chunk_start ? a.chunk_start[r] : (int64_t)r * F;
    const float *px = a.soa + ((int64_t)v * 3 + 0) * a.Npad + start;
    const float *py = px + a.Npad;
    const float *pz = py + a.Npad;
    cplx *fb = lds + tid + (tid >> 3);                 // frequency / natural order: element tid + 256 j + 32 N1 k'

    double W[G][8];
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) W[j][e] = 0.0;

    // three packed pairs: (x^2, y^2) weights 1,1; (z^2, xy) weights 1,2; (xz, yz) weights 2,2.  The samples are
    // re-read from the planes for every pair (L2 hits) rather than kept in 96 registers across the transforms.
#pragma unroll 1
    for (int pair = 0; pair < 3; ++pair) {
        // the samples are re-read for every pair (L2 hits; keeping them in registers across the loop makes the
        // compiler hoist all six products, 384 VGPRs).  All 3 N1 loads are issued before the first use -- with one
        // wave per SIMD a load-use-load-use sequence pays the memory latency N1 times (1.5 ms of 3.6 ms).
        asm volatile("" ::: "memory");
        float xr[N1], yr[N1], zr[N1];
#pragma unroll
        for (int n1 = 0; n1 < N1; ++n1) {
            if (n1 >= NZ) {
                xr[n1] = yr[n1] = zr[n1] = 0.f;
                continue;
            }
            const int n = tid + 256 * n1;
            const bool in = n < F;
            // unconditional loads from a clamped index + select: a conditional load becomes a branch, and a branch per
            // sample serialises the memory latency (that alone was 1.5 ms of 3.6 ms)
            const int nc = in ? n : 0;
            const float xv = px[nc], yv = py[nc], zv = pz[nc];
            xr[n1] = in ? xv : 0.f;
            yr[n1] = in ? yv : 0.f;
            zr[n1] = in ? zv : 0.f;
        }
        cplx sig[N1];
#pragma unroll
        for (int n1 = 0; n1 < N1; ++n1) {
            const double x = (double)xr[n1], y = (double)yr[n1], z = (double)zr[n1];
            if (pair == 0) sig[n1] = {x * x, y * y};
            else if (pair == 1) sig[n1] = {z * z, x * y};
            else sig[n1] = {x * z, y * z};
        }
        cplx w[G][8];
        fft_workgroup<N1>(sig, w, lds, a.tab, tid);
        // spectrum to LDS in frequency order, then every thread reads the mirror frequency of its own ones
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int p = 0; p < 8; ++p) fb[fft_pad(256 * j + 32 * N1 * bitrev<3>(p))] = w[j][p];
        __syncthreads();
        const double wp = pair == 2 ? 2.0 : 1.0, wq = pair == 0 ? 1.0 : 2.0;
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int k = tid + 256 * j + 32 * N1 * bitrev<3>(p);
                const int km = k == 0 ? 0 : M - k;
                const cplx zm = lds[km + (km >> 3) + 8 * (km >> 8)];
                const cplx zk = w[j][p];
                // P = (Z(k) + conj Z(M-k)) / 2, Q = (Z(k) - conj Z(M-k)) / (2i)
                const double sr = zk.re + zm.re, si = zk.im - zm.im;
                const double dr = zk.re - zm.re, di = zk.im + zm.im;
                W[j][p] += 0.25 * (wp * (sr * sr + si * si) + wq * (dr * dr + di * di));
            }
        __syncthreads();
    }
    // the weighted power spectrum (real, even) back through the same transform
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
        for (int p = 0; p < 8; ++p) fb[fft_pad(256 * j + 32 * N1 * bitrev<3>(p))] = {W[j][p], 0.0};
    __syncthreads();
    {
        cplx sig[N1];
#pragma unroll
        for (int n1 = 0; n1 < N1; ++n1) sig[n1] = fb[fft_pad(256 * n1)];
        __syncthreads();
        cplx w[G][8];
        fft_workgroup<N1>(sig, w, lds, a.tab, tid);
        double *out = a.psum + ((int64_t)v * a.R + r) * a.Lp;
        const double inv = 1.0 / (double)M;
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int lag = tid + 256 * j + 32 * N1 * bitrev<3>(p);
                if (lag >= 1 && lag <= a.L) out[lag] = w[j][p].re * inv;
            }
    }
}

template <int N1, bool HALF>
int launch_ct_fft_h(sr_ctx *ctx, const CtFftArgs &a, int64_t series)
{
    return sr_launch(ctx, k_ct_fft<N1, HALF>, dim3((unsigned)series), dim3(256), (size_t)fft_lds_slots(256 * N1) * sizeof(cplx), a);
}
// The transform length follows from need = F + L = F + F/2, and with it what HALF can be.  N1 = 24 runs for 4096 < need <= 6144,
// i.e. F <= 4096 = 256 * 16: always HALF.  N1 = 32 runs for need > 6144, i.e. F >= 4097 > 256 * 16: never.  Only N1 = 8 and 16
// see chunks on both sides of 256 NZ, so <24, false> and <32, true> are not instantiated.
template <int N1>
int launch_ct_fft(sr_ctx *ctx, const CtFftArgs &a, int64_t series)
{
    if constexpr (N1 == 24) return launch_ct_fft_h<24, true>(ctx, a, series);
    else if constexpr (N1 == 32) return launch_ct_fft_h<32, false>(ctx, a, series);
    else return a.F <= 256 * (N1 / 2) ? launch_ct_fft_h<N1, true>(ctx, a, series) : launch_ct_fft_h<N1, false>(ctx, a, series);
}

}  // namespace

const void *sr_ct64_table(sr_ctx *ctx)
{
    Ct64Tab *tab = (Ct64Tab *)sr_workspace(ctx, SR_WS_FFT, sizeof(Ct64Tab));
    if (!tab) return nullptr;
    if (!ctx->fft_table_ready) {
        hipLaunchKernelGGL(k_fft_init_table, dim3((kFftTabDoubles / 2 + 255) / 256), dim3(256), 0, ctx->stream, reinterpret_cast<double *>(tab));
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // once per context: later launches may come on other streams
        if (e != hipSuccess) { sr_set_error("k_fft_init_table -> %s", hipGetErrorString(e)); return nullptr; }
        ctx->fft_table_ready = 1;
    }
    return tab;
}

// Called by sr_ct_palmer_sums_f32_dev (sr_ct.hip) for 1024 < F + L <= 8192.
int sr_launch_ct_fft64(sr_ctx *ctx, const sr_ct_job &j)
{
    CtFftArgs a;
    a.soa = j.soa; a.Npad = j.Npad; a.chunk_start = j.cs_dev; a.psum = j.psum;
    a.R = j.R; a.F = j.F; a.L = j.L; a.Lp = j.Lp;
    if (!(a.tab = (const Ct64Tab *)sr_ct64_table(ctx))) return -5;
    const int need = j.F + j.L;
    SR_REQUIRE(need > 1024 && need <= 8192, -3, "k_ct_fft: F=%d outside the transform lengths", j.F);
    return need <= 2048 ? launch_ct_fft<8>(ctx, a, j.series)
           : need <= 4096 ? launch_ct_fft<16>(ctx, a, j.series)
           : need <= 6144 ? launch_ct_fft<24>(ctx, a, j.series) : launch_ct_fft<32>(ctx, a, j.series);
}
