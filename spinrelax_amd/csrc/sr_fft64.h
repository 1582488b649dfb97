// sr_fft64.h -- the float64 pieces that k_ct_fft (sr_ct_fft64.hip) and k_ct_rfft (sr_ct_rfft64.hip) share: complex arithmetic, the
// in-register transforms (radix 2 up to 32 points; the step-1 transforms of each kernel, 24 = 3 x 8 and 12 = 3 x 4 among them),
// the layout of the context's twiddle table, and the complex workgroup transform of 256 N1 points (fft_workgroup) that k_ct_fft shares
// with k_ired_mode_ct (sr_ired_modes.hip).  What is independent of the scalar type: sr_fft_common.h.
#pragma once
#include <cstddef>
#include "sr_fft_common.h"

namespace {

struct cplx {
    double re, im;
};
__device__ __forceinline__ cplx cmul(cplx a, cplx b)
{
    return {fma(a.re, b.re, -(a.im * b.im)), fma(a.re, b.im, a.im * b.re)};
}

// d * exp(-2 pi i e / 32), e a compile-time constant after unrolling
template <int E>
__device__ __forceinline__ cplx mul_w32(cplx d)
{
    if (E == 0) return d;
    if (E == 8) return {d.im, -d.re};
    constexpr double c[16] = {1.0, 0.9807852804032304, 0.9238795325112867, 0.8314696123025452, 0.7071067811865476,
                              0.5555702330196023, 0.38268343236508984, 0.19509032201612833, 0.0,
                              -0.1950903220161282, -0.3826834323650897, -0.555570233019602, -0.7071067811865475,
                              -0.8314696123025453, -0.9238795325112867, -0.9807852804032304};
    constexpr double s[16] = {0.0, 0.19509032201612825, 0.3826834323650898, 0.5555702330196022, 0.7071067811865475,
                              0.8314696123025452, 0.9238795325112867, 0.9807852804032304, 1.0, 0.9807852804032304,
                              0.9238795325112867, 0.8314696123025455, 0.7071067811865476, 0.5555702330196022,
                              0.3826834323650899, 0.1950903220161286};
    return {fma(d.re, c[E], d.im * s[E]), fma(d.im, c[E], -(d.re * s[E]))};
}

// d * exp(-2 pi i e / 32) for e = 0..15 known after unrolling (a switch the optimiser folds)
__device__ __forceinline__ cplx mul_w32_rt(cplx d, int e)
{
    switch (e) {
        case 0: return mul_w32<0>(d);
        case 1: return mul_w32<1>(d);
        case 2: return mul_w32<2>(d);
        case 3: return mul_w32<3>(d);
        case 4: return mul_w32<4>(d);
        case 5: return mul_w32<5>(d);
        case 6: return mul_w32<6>(d);
        case 7: return mul_w32<7>(d);
        case 8: return mul_w32<8>(d);
        case 9: return mul_w32<9>(d);
        case 10: return mul_w32<10>(d);
        case 11: return mul_w32<11>(d);
        case 12: return mul_w32<12>(d);
        case 13: return mul_w32<13>(d);
        case 14: return mul_w32<14>(d);
        default: return mul_w32<15>(d);
    }
}

template <int LOGN, int S, int BLK, int J>
struct FftStage {
    __device__ static __forceinline__ void run(cplx *v)
    {
        constexpr int N = 1 << LOGN;
        constexpr int half = N >> (S + 1);
        constexpr int i = BLK * 2 * half + J;
        const cplx a = v[i], b = v[i + half];
        v[i] = {a.re + b.re, a.im + b.im};
        const cplx d = {a.re - b.re, a.im - b.im};
        v[i + half] = mul_w32<((J << S) * (32 / N)) & 15>(d);
        if constexpr (J + 1 < half) FftStage<LOGN, S, BLK, J + 1>::run(v);
        else if constexpr (BLK + 1 < (1 << S)) FftStage<LOGN, S, BLK + 1, 0>::run(v);
        else if constexpr (S + 1 < LOGN) FftStage<LOGN, S + 1, 0, 0>::run(v);
    }
};
// in-register radix-2 decimation-in-frequency transform of N = 2^LOGN <= 32 points; v[p] ends up holding X[rev(p)]
template <int LOGN>
__device__ __forceinline__ void fft_reg(cplx *v)
{
    FftStage<LOGN, 0, 0, 0>::run(v);
}
// d * exp(-2 pi i e / 24), e a compile-time constant
template <int E>
__device__ __forceinline__ cplx mul_w24(cplx d)
{
    if (E == 0) return d;
    if (E == 6) return {d.im, -d.re};
    if (E == 12) return {-d.re, -d.im};
    constexpr double c[15] = {1.0, 0.9659258262890683, 0.8660254037844387, 0.7071067811865476, 0.5000000000000001,
                              0.25881904510252074, 0.0, -0.25881904510252063, -0.4999999999999998, -0.7071067811865475,
                              -0.8660254037844387, -0.9659258262890682, -1.0, -0.9659258262890683, -0.8660254037844388};
    constexpr double s[15] = {0.0, 0.25881904510252074, 0.49999999999999994, 0.7071067811865475, 0.8660254037844386,
                              0.9659258262890683, 1.0, 0.9659258262890683, 0.8660254037844387, 0.7071067811865476,
                              0.49999999999999994, 0.258819045102521, 0.0, -0.2588190451025208, -0.4999999999999997};
    return {fma(d.re, c[E], d.im * s[E]), fma(d.im, c[E], -(d.re * s[E]))};
}

// First stage of the four-step transform: N1 samples per thread -> N1 frequencies k1, in place; v[p] holds X[k1(p)].
template <int N1>
struct Stage1 : Stage1Map<N1> {                            // N1 = 8, 16, 32
    __device__ static __forceinline__ void run(cplx *v) { fft_reg<Stage1Map<N1>::LOG>(v); }
};
// 24 = 3 x 8 (transform length 6144 = F + L for the F = 4096 chunks: a quarter less work than 8192): n1 = 8 a + b,
// k1 = ka + 3 kb; 3-point transforms over a, twiddle w_24^(b ka), 8-point transforms over b
template <int B>
__device__ __forceinline__ void dft3_col(cplx *v, cplx (*y)[8])
{
    constexpr double h = 0.8660254037844386;            // sqrt(3)/2
    const cplx x0 = v[B], x1 = v[8 + B], x2 = v[16 + B];
    const cplx t = {x1.re + x2.re, x1.im + x2.im}, d = {x1.re - x2.re, x1.im - x2.im};
    const cplx m = {fma(-0.5, t.re, x0.re), fma(-0.5, t.im, x0.im)};
    const cplx r = {h * d.im, -h * d.re};                // -i sqrt(3)/2 (x1 - x2)
    y[0][B] = {x0.re + t.re, x0.im + t.im};
    y[1][B] = mul_w24<B>(cplx{m.re + r.re, m.im + r.im});
    y[2][B] = mul_w24<2 * B>(cplx{m.re - r.re, m.im - r.im});
    if constexpr (B + 1 < 8) dft3_col<B + 1>(v, y);
}
template <>
struct Stage1<24> {
    __host__ __device__ static constexpr int k1(int p) { return (p >> 3) + 3 * bitrev<3>(p & 7); }
    __device__ static __forceinline__ void run(cplx *v)
    {
        cplx y[3][8];
        dft3_col<0>(v, y);
#pragma unroll
        for (int ka = 0; ka < 3; ++ka) {
            fft_reg<3>(y[ka]);
#pragma unroll
            for (int q = 0; q < 8; ++q) v[8 * ka + q] = y[ka][q];
        }
    }
};

// The same for the half-length transforms of k_ct_rfft: 16, and 12 = 3 x 4
template <int N1>
struct RStage1 : Stage1Map<N1> {                           // N1 = 16
    __device__ static __forceinline__ void run(cplx *v) { fft_reg<Stage1Map<N1>::LOG>(v); }
};
template <int B>
__device__ __forceinline__ void dft3_col12(cplx *v, cplx (*y)[4])
{
    constexpr double h = 0.8660254037844386;            // sqrt(3)/2
    const cplx x0 = v[B], x1 = v[4 + B], x2 = v[8 + B];
    const cplx t = {x1.re + x2.re, x1.im + x2.im}, d = {x1.re - x2.re, x1.im - x2.im};
    const cplx m = {fma(-0.5, t.re, x0.re), fma(-0.5, t.im, x0.im)};
    const cplx r = {h * d.im, -h * d.re};                // -i sqrt(3)/2 (x1 - x2)
    y[0][B] = {x0.re + t.re, x0.im + t.im};
    y[1][B] = mul_w24<2 * B>(cplx{m.re + r.re, m.im + r.im});          // w_12^B
    y[2][B] = mul_w24<4 * B>(cplx{m.re - r.re, m.im - r.im});          // w_12^(2B)
    if constexpr (B + 1 < 4) dft3_col12<B + 1>(v, y);
}
template <>
struct RStage1<12> : Stage1Map<12> {
    __device__ static __forceinline__ void run(cplx *v)
    {
        cplx y[3][4];
        dft3_col12<0>(v, y);
#pragma unroll
        for (int ka = 0; ka < 3; ++ka) {
            fft_reg<2>(y[ka]);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[4 * ka + q] = y[ka][q];
        }
    }
};


// Hide a value's provenance from the optimiser.  Twiddle bases depend only on the thread, so everything derived from them
// (11 + 15 + 16 complex powers) is invariant across the six transforms of a series: left alone, the compiler computes them
// once, parks 100+ registers and spills them (83 scratch stores in the prologue, ~150 reloads per transform; the kernel
// then waits on scratch 85 % of the time).  Recomputing them per transform is a few dozen multiplies.
__device__ __forceinline__ cplx opaque(cplx z)
{
    asm volatile("" : "+v"(z.re), "+v"(z.im));
    return z;
}
// (The same for the thread index: opaque(int), sr_fft_common.h.)

// The twiddle table of a context, one workspace slot: every entry a pair (cos, -sin), i.e. w_N^t = exp(-2 pi i t / N)
struct Ct64Tab {
    double w8192[2 * 1024];          // k_ct_fft, N1 a power of two: w_8192^t, t < 1024
    double w6144[2 * 256];           // k_ct_fft<24>: w_6144^t, t < 256 (the kernel reaches it as entry 1024 + t of w8192)
    struct Rfft {                    // k_ct_rfft: three tables of 256, H = 256 N1, M = 2 H
        double wH[2 * 256];          // w_H^t
        double w256[2 * 256];        // w_256^t
        double wM[2 * 256];          // w_M^t
    } rfft[2];                       // N1 = 12, N1 = 16
};
constexpr int kFftTabDoubles = sizeof(Ct64Tab) / sizeof(double);
// the table as the flat array of complex entries that Ct64Tab lays out: t < 1280 the two k_ct_fft tables, then 2 x 3 x 256
static_assert(offsetof(Ct64Tab, w6144) == 2 * 1024 * sizeof(double) && offsetof(Ct64Tab, rfft) == 2 * 1280 * sizeof(double) &&
              sizeof(Ct64Tab::Rfft) == 2 * 768 * sizeof(double) && kFftTabDoubles == 2 * (1280 + 2 * 768), "k_fft_init_table's indexing");

// ---- the complex workgroup transform of M = 256 N1 points (k_ct_fft, sr_ct_fft64.hip; k_ired_mode_ct, sr_ired_modes.hip) ----
// v[p] *= base^k(p), k(p) < N: base^k = A[k & 7] * B[k >> 3] with 8 + N/8 powers held in registers (a full table of N
// powers would cost 4 N VGPRs next to the 4 N of the data)
template <int N, class KOF>
__device__ __forceinline__ void apply_twiddles(cplx *v, cplx base)
{
    constexpr int NA = N < 8 ? N : 8, NB = N / 8 > 0 ? N / 8 : 1;
    cplx A[NA], B[NB];
    A[0] = {1.0, 0.0};
#pragma unroll
    for (int k = 1; k < NA; ++k) A[k] = k == 1 ? base : cmul(A[k >> 1], A[k - (k >> 1)]);
    B[0] = {1.0, 0.0};
    if (NB > 1) {
        B[1] = cmul(A[4], A[4]);
#pragma unroll
        for (int k = 2; k < NB; ++k) B[k] = cmul(B[k >> 1], B[k - (k >> 1)]);
    }
#pragma unroll
    for (int p = 0; p < N; ++p) {
        const int k = KOF::k1(p);
        if (k == 0) continue;
        const cplx t = (k >> 3) == 0 ? A[k & 7] : ((k & 7) == 0 ? B[k >> 3] : cmul(A[k & 7], B[k >> 3]));
        v[p] = cmul(v[p], t);
    }
}

// LDS slot of logical element a: one pad slot per 8 elements and eight per 256.  Every access pattern below splits into
// a per-thread part and a compile-time part without carries between them, so each access is `base + immediate`.
__host__ __device__ constexpr int fft_pad(int a) { return a + (a >> 3) + 8 * (a >> 8); }
__host__ __device__ constexpr int fft_lds_slots(int M) { return M + (M >> 3) + 8 * (M >> 8); }

// one full transform of the thread's N1 samples v[] (natural order, sample n = tid + 256 n1) -> the thread's
// G = N1/8 groups of 8 spectrum values w[j][p] = X[g + 32 N1 rev3(p)], g = tid + 256 j.  Ends with a barrier.
template <int N1>
__device__ __forceinline__ void fft_workgroup(cplx *v, cplx (*w)[8], cplx *lds, const Ct64Tab *__restrict__ tab, int tid)
{
    constexpr int G = N1 / 8;
    constexpr bool kPow2 = (N1 & (N1 - 1)) == 0;
    // step 1: N1-point transforms over n1, twiddle w_M^(n2 k1), to LDS as element k1*256 + n2
    Stage1<N1>::run(v);
    {
        const double *tw = kPow2 ? tab->w8192 + 2 * (8192 / (N1 * 256)) * tid : tab->w6144 + 2 * tid;      // w_M^tid
        apply_twiddles<N1, Stage1<N1>>(v, cplx{tw[0], tw[1]});
        cplx *b = lds + tid + (tid >> 3);
#pragma unroll
        for (int p = 0; p < N1; ++p) b[fft_pad(Stage1<N1>::k1(p) * 256)] = v[p];
    }
    __syncthreads();
    // step 2: thread (k1, lo), active while k1 < N1: 32-point transforms over h (n2 = lo + 8 h), twiddle w_256^(lo k2a)
    cplx u[32];
    const int k1 = tid >> 3, lo = tid & 7;
    const bool act = k1 < N1;
    if (act) {
        const cplx *b = lds + fft_pad(256) * k1 + lo;
#pragma unroll
        for (int h = 0; h < 32; ++h) u[h] = b[9 * h];
        fft_reg<5>(u);
        apply_twiddles<32, Stage1<32>>(u, cplx{tab->w8192[2 * (32 * lo)], tab->w8192[2 * (32 * lo) + 1]});
    }
    __syncthreads();
    if (act) {
        // element (k1 + N1 k2a)*8 + lo
        if constexpr (kPow2) {
            cplx *b = lds + 9 * k1 + lo;
#pragma unroll
            for (int p = 0; p < 32; ++p) b[fft_pad(8 * N1 * bitrev<5>(p))] = u[p];
        } else {
            // 8 N1 is not a power of two: the per-thread and the constant part of the slot can carry into each other
            const int t = 8 * k1 + lo;
#pragma unroll
            for (int p = 0; p < 32; ++p) {
                const int c = 8 * N1 * bitrev<5>(p);
                lds[t + c + ((t + c) >> 3) + 8 * ((t + c) >> 8)] = u[p];
            }
        }
    }
    __syncthreads();
    // step 3: thread q, groups g = q + 256 j: 8-point transforms over lo
    {
        const cplx *b = lds + 9 * tid + 8 * (tid >> 5);
#pragma unroll
        for (int j = 0; j < G; ++j) {
#pragma unroll
            for (int e = 0; e < 8; ++e) w[j][e] = b[fft_pad(2048 * j) + e];
            fft_reg<3>(w[j]);
        }
    }
    __syncthreads();
}

}  // namespace

// the context's table (a Ct64Tab on the device), created on first use; NULL (error set) on failure.  sr_ct_fft64.hip
const void *sr_ct64_table(sr_ctx *ctx);
