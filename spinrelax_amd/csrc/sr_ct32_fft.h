// sr_ct32_fft.h -- device functions of the float32 transforms of kernel 1, shared by sr_ct32.hip (k_ct_rfft32: one transform per
// series) and sr_ct_long.hip (the blocked form for long chunks): packed complex arithmetic, the in-register butterflies, the
// workgroup transform of half length 256 N1, its tables, and the one definition of the transforms' inputs.  Index maps, image
// size and wave scans: sr_fft_common.h.
#pragma once
#include "sr_fft_common.h"
#include "sr_pack_tile.h"

namespace {

// ---- packed complex float32 arithmetic ------------------------------------------------------------------------------
// A complex number is one 64-bit register pair (re, im) and every operation below is ONE or TWO v_pk_*_f32 instructions.
// Why it matters (scripts/dev/probe/pk_rate.hip, profiles/r05_pk_issue_rate.txt): a gfx950 wave issues a plain float32
// VALU instruction every ~6 cycles whatever its neighbours do, a packed one every ~7 -- twice the arithmetic per issue; the SIMD
// only saturates on plain instructions with three waves issuing at once, and this kernel, with its barriers and LDS round
// trips, has about one.  (Left to the SLP vectoriser the packing costs a v_mov per operand pair and 270 B of scratch; here
// the swaps and sign flips of complex arithmetic ride on the op_sel / neg modifiers, spelled out in inline assembly where
// the compiler does not fold them itself.)
typedef float c32 __attribute__((ext_vector_type(2)));     // .x = re, .y = im
#define SR_PK __device__ __forceinline__
SR_PK c32 pk_fma(c32 a, c32 b, c32 c) { return __builtin_elementwise_fma(a, b, c); }
SR_PK c32 splat(float c) { return c32{c, c}; }
// a + (-i) b = (a.re + b.im, a.im - b.re)
SR_PK c32 add_mi(c32 a, c32 b)
{
    c32 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a + i b = (a.re - b.im, a.im + b.re)
SR_PK c32 add_pi(c32 a, c32 b)
{
    c32 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// (-i) (a - b) = (a.im - b.im, b.re - a.re)
SR_PK c32 mi_sub(c32 a, c32 b)
{
    c32 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,0] neg_lo:[0,1] neg_hi:[1,0]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a + conj(b), a - conj(b)
SR_PK c32 add_conj(c32 a, c32 b)
{
    c32 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
SR_PK c32 sub_conj(c32 a, c32 b)
{
    c32 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// (s.re + t.im, s.re - t.im) and (s.im - t.re, s.im + t.re): real and imaginary parts of the pair (s - i t, s + i t)
SR_PK c32 pair_re(c32 s, c32 t)
{
    c32 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(s), "v"(t));
    return r;
}
SR_PK c32 pair_im(c32 s, c32 t)
{
    c32 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(s), "v"(t));
    return r;
}
// a * w, both variable
SR_PK c32 cmulf(c32 a, c32 w)
{
    c32 t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0]" : "=v"(t) : "v"(a), "v"(w));                       // (a.im w.im, a.im w.re)
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1] neg_lo:[0,0,1]" : "=v"(r) : "v"(a), "v"(w), "v"(t));
    return r;
}
// a1 *= w1, a2 *= w2 as ONE block: a packed instruction that consumes the result of the packed instruction right before it costs
// a wait state (the compiler puts an s_nop between the two halves of cmulf); two products interleaved need none.
SR_PK void cmulf2(c32 &a1, c32 w1, c32 &a2, c32 w2)
{
    c32 t1, t2;
    asm("v_pk_mul_f32 %2, %0, %4 op_sel:[1,1] op_sel_hi:[1,0]\n\t"
        "v_pk_mul_f32 %3, %1, %5 op_sel:[1,1] op_sel_hi:[1,0]\n\t"
        "v_pk_fma_f32 %0, %0, %4, %2 op_sel:[0,0,0] op_sel_hi:[0,1,1] neg_lo:[0,0,1]\n\t"
        "v_pk_fma_f32 %1, %1, %5, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1] neg_lo:[0,0,1]"
        : "+v"(a1), "+v"(a2), "=&v"(t1), "=&v"(t2) : "v"(w1), "v"(w2));
}
// d * (C - i S), C and S compile-time constants: (d.re C + d.im S, d.im C - d.re S)
template <int CBITS, int SBITS>
SR_PK c32 mul_const(c32 d)
{
    const float C = __builtin_bit_cast(float, CBITS), S = __builtin_bit_cast(float, SBITS);
    return pk_fma(d.yx, c32{S, -S}, d * splat(C));
}
constexpr int fbits(float f) { return __builtin_bit_cast(int, f); }

// d * exp(-2 pi i E / 32), E a compile-time constant
template <int E>
SR_PK c32 mulf_w32(c32 d)
{
    constexpr float c[16] = {1.0f, 0.9807852804032304f, 0.9238795325112867f, 0.8314696123025452f, 0.7071067811865476f,
                             0.5555702330196023f, 0.38268343236508984f, 0.19509032201612833f, 0.0f,
                             -0.1950903220161282f, -0.3826834323650897f, -0.555570233019602f, -0.7071067811865475f,
                             -0.8314696123025453f, -0.9238795325112867f, -0.9807852804032304f};
    constexpr float s[16] = {0.0f, 0.19509032201612825f, 0.3826834323650898f, 0.5555702330196022f, 0.7071067811865475f,
                             0.8314696123025452f, 0.9238795325112867f, 0.9807852804032304f, 1.0f, 0.9807852804032304f,
                             0.9238795325112867f, 0.8314696123025455f, 0.7071067811865476f, 0.5555702330196022f,
                             0.3826834323650899f, 0.1950903220161286f};
    if constexpr (E == 0) return d;
    else if constexpr (E == 8) return c32{d.y, -d.x};
    else if constexpr (E == 4) return add_mi(d, d) * splat(c[4]);              // sqrt(1/2) (d.re + d.im, d.im - d.re)
    else if constexpr (E == 12) return add_pi(d, d) * splat(-c[4]);            // -sqrt(1/2) (d.re - d.im, d.im + d.re)
    else return mul_const<fbits(c[E]), fbits(s[E])>(d);
}
SR_PK c32 mulf_w32_rt(c32 d, int e)      // e = 0..15 known after unrolling
{
    switch (e) {
        case 0: return mulf_w32<0>(d);
        case 1: return mulf_w32<1>(d);
        case 2: return mulf_w32<2>(d);
        case 3: return mulf_w32<3>(d);
        case 4: return mulf_w32<4>(d);
        case 5: return mulf_w32<5>(d);
        case 6: return mulf_w32<6>(d);
        case 7: return mulf_w32<7>(d);
        case 8: return mulf_w32<8>(d);
        case 9: return mulf_w32<9>(d);
        case 10: return mulf_w32<10>(d);
        case 11: return mulf_w32<11>(d);
        case 12: return mulf_w32<12>(d);
        case 13: return mulf_w32<13>(d);
        case 14: return mulf_w32<14>(d);
        default: return mulf_w32<15>(d);
    }
}
// d * exp(-2 pi i E / 24)
template <int E>
SR_PK c32 mulf_w24(c32 d)
{
    constexpr float c[15] = {1.0f, 0.9659258262890683f, 0.8660254037844387f, 0.7071067811865476f, 0.5000000000000001f,
                             0.25881904510252074f, 0.0f, -0.25881904510252063f, -0.4999999999999998f, -0.7071067811865475f,
                             -0.8660254037844387f, -0.9659258262890682f, -1.0f, -0.9659258262890683f, -0.8660254037844388f};
    constexpr float s[15] = {0.0f, 0.25881904510252074f, 0.49999999999999994f, 0.7071067811865475f, 0.8660254037844386f,
                             0.9659258262890683f, 1.0f, 0.9659258262890683f, 0.8660254037844387f, 0.7071067811865476f,
                             0.49999999999999994f, 0.258819045102521f, 0.0f, -0.2588190451025208f, -0.4999999999999997f};
    if constexpr (E == 0) return d;
    else if constexpr (E == 6) return c32{d.y, -d.x};
    else if constexpr (E == 12) return -d;
    else return mul_const<fbits(c[E]), fbits(s[E])>(d);
}

template <int LOGN, int S, int BLK, int J>
struct FftStageF {
    __device__ static __forceinline__ void run(c32 *v)
    {
        constexpr int N = 1 << LOGN;
        constexpr int half = N >> (S + 1);
        constexpr int i = BLK * 2 * half + J;
        constexpr int E = ((J << S) * (32 / N)) & 15;
        const c32 a = v[i], b = v[i + half];
        v[i] = a + b;
        if constexpr (E == 8) v[i + half] = mi_sub(a, b);              // the -i of the twiddle rides on the subtraction
        else v[i + half] = mulf_w32<E>(a - b);
        if constexpr (J + 1 < half) FftStageF<LOGN, S, BLK, J + 1>::run(v);
        else if constexpr (BLK + 1 < (1 << S)) FftStageF<LOGN, S, BLK + 1, 0>::run(v);
        else if constexpr (S + 1 < LOGN) FftStageF<LOGN, S + 1, 0, 0>::run(v);
    }
};
// in-register radix-2 decimation-in-frequency transform of N = 2^LOGN <= 16 points; v[p] ends up holding X[rev(p)]
template <int LOGN>
__device__ __forceinline__ void fftf_reg(c32 *v)
{
    FftStageF<LOGN, 0, 0, 0>::run(v);
}

template <int N1>
struct FStage1 : Stage1Map<N1> {                           // N1 = 4, 8, 16
    __device__ static __forceinline__ void run(c32 *v) { fftf_reg<Stage1Map<N1>::LOG>(v); }
};
template <int B>
__device__ __forceinline__ void dft3f_col12(c32 *v, c32 (*y)[4])
{
    constexpr float h = 0.8660254037844386f;             // sqrt(3)/2
    const c32 x0 = v[B], x1 = v[4 + B], x2 = v[8 + B];
    const c32 t = x1 + x2, d = x1 - x2;
    const c32 m = pk_fma(splat(-0.5f), t, x0);
    const c32 hd = d * splat(h);
    y[0][B] = x0 + t;
    y[1][B] = mulf_w24<2 * B>(add_mi(m, hd));              // w_12^B (m - i h d)
    y[2][B] = mulf_w24<4 * B>(add_pi(m, hd));              // w_12^(2B) (m + i h d)
    if constexpr (B + 1 < 4) dft3f_col12<B + 1>(v, y);
}
template <>
struct FStage1<12> : Stage1Map<12> {
    __device__ static __forceinline__ void run(c32 *v)
    {
        c32 y[3][4];
        dft3f_col12<0>(v, y);
#pragma unroll
        for (int ka = 0; ka < 3; ++ka) {
            fftf_reg<2>(y[ka]);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[4 * ka + q] = y[ka][q];
        }
    }
};

// Hide a value's provenance from the optimiser (see k_ct_rfft, sr_ct_fft64.hip: thread-invariant twiddles would otherwise be
// computed once per kernel, parked in registers the loop does not have, and spilled).  The thread index: opaque(), sr_fft_common.h.
__device__ __forceinline__ c32 opaquef(c32 z)
{
    asm volatile("" : "+v"(z));
    return z;
}

// v[p] *= base^k(p), base = w_H^tid.  The thread reads base^1, base^2, base^4, base^8 from four float32 tables (each entry
// rounded once from float64) and multiplies them up: k = 3, 5, 6, 9, 10, 12 cost one float32 complex multiply (one more
// rounding), 7, 11, 13, 14 two, 15 three -- against four levels of a multiply tree started from base alone, and against 43
// float64 instructions + 22 conversions per transform for exactly rounded powers.
template <int N, class KOF>
__device__ __forceinline__ void applyf_twiddles(c32 *v, const c32 *tw, int tid)
{
    c32 pw[16];
    pw[1] = opaquef(tw[tid]);
    pw[2] = opaquef(tw[256 + tid]);
    pw[4] = opaquef(tw[512 + tid]);
    pw[8] = opaquef(tw[768 + tid]);
    static_assert(N == 4 || N == 8 || N == 12 || N == 16, "the step-1 sizes");
    static_assert(KOF::k1(0) == 0, "entry 0 carries no twiddle");
    if constexpr (N == 4) {                                // k1(p) = 0, 2, 1, 3
        pw[3] = cmulf(pw[1], pw[2]);
        cmulf2(v[1], pw[2], v[2], pw[1]);
        v[3] = cmulf(v[3], pw[3]);
        return;
    } else if constexpr (N == 8) {                         // k1(p) = 0, 4, 2, 6, 1, 5, 3, 7
        pw[3] = pw[1]; pw[5] = pw[1];
        cmulf2(pw[3], pw[2], pw[5], pw[4]);
        pw[6] = pw[2]; pw[7] = pw[3];
        cmulf2(pw[6], pw[4], pw[7], pw[4]);
        v[1] = cmulf(v[1], pw[4]);
#pragma unroll
        for (int p = 2; p + 1 < N; p += 2) cmulf2(v[p], pw[KOF::k1(p)], v[p + 1], pw[KOF::k1(p + 1)]);
        return;
    }
    pw[3] = pw[1]; pw[5] = pw[1]; pw[6] = pw[2]; pw[9] = pw[1]; pw[10] = pw[2];
    cmulf2(pw[3], pw[2], pw[5], pw[4]);
    cmulf2(pw[6], pw[4], pw[9], pw[8]);
    pw[7] = pw[3]; pw[11] = pw[3];
    if constexpr (N == 12) {
        cmulf2(pw[10], pw[8], pw[7], pw[4]);
        cmulf2(pw[11], pw[8], v[1], pw[KOF::k1(1)]);       // k1(1) = 6
    } else {
        pw[12] = pw[4];
        cmulf2(pw[10], pw[8], pw[12], pw[8]);
        pw[13] = pw[5]; pw[14] = pw[6];
        cmulf2(pw[7], pw[4], pw[11], pw[8]);
        cmulf2(pw[13], pw[8], pw[14], pw[8]);
        pw[15] = pw[7];
        cmulf2(pw[15], pw[8], v[1], pw[KOF::k1(1)]);       // k1(1) = 8
    }
    // v[p] *= pw[k1(p)], two at a time (p = 0 carries no twiddle, p = 1 went with the last power)
#pragma unroll
    for (int p = 2; p + 1 < N; p += 2) cmulf2(v[p], pw[KOF::k1(p)], v[p + 1], pw[KOF::k1(p + 1)]);
}

// Tables (computed in float64, rounded once; per N1): w_H^(j t) for j = 1, 2, 4, 8 (step-1 twiddle bases), w_256^t, w_M^t, t < 256
struct Ct32Tab {
    float w1[4][2 * 256];
    float w2[2 * 256];
    float w3[2 * 256];
};
__host__ __device__ constexpr int f32_tab_set(int N1) { return N1 / 4 - 1; }       // N1 = 4, 8, 12, 16 -> 0 .. 3
__global__ void k_ct32_init_table(Ct32Tab *tab)          // tab[N1 / 4 - 1], H = 256 N1
{
    const int t = threadIdx.x, set = blockIdx.x;
    const double H = 1024.0 * (double)(set + 1);
    double sn, cs;
    for (int j = 0; j < 4; ++j) {
        const int e = (t << j) % (int)H;                   // exact argument reduction
        sincospi(2.0 * (double)e / H, &sn, &cs);
        tab[set].w1[j][2 * t] = (float)cs;
        tab[set].w1[j][2 * t + 1] = (float)-sn;
    }
    sincospi(2.0 * (double)t / 256.0, &sn, &cs);
    tab[set].w2[2 * t] = (float)cs;
    tab[set].w2[2 * t + 1] = (float)-sn;
    sincospi((double)t / H, &sn, &cs);
    tab[set].w3[2 * t] = (float)cs;
    tab[set].w3[2 * t + 1] = (float)-sn;
}

struct Ct32Args {
    const float *soa;
    int64_t Npad;
    const int64_t *chunk_start;   // device, may be null
    const Ct32Tab *tab;
    double *psum;                 // (nV, R, Lp)
    int R, F, L, Lp;
    sr_pack_job pk;               // k_ct_rfft32<.., .., true> only: the next batch's pack, carried by this launch (sr_pack_tile.h)
};

#ifdef SR_CT32_STAMPS           // development: s_memtime stamps around the phases of a pass, summed per wave, left behind lag L of the
#define SR_STAMP(I) { const long long t_ = __builtin_amdgcn_s_memtime(); stamp_acc[I] += t_ - stamp_t; stamp_t = t_; }   // series' sums
#else
#define SR_STAMP(I)
#endif
#ifdef SR_CT32_EXP_NOBAR        // timing experiment: no workgroup barriers (wrong results)
#define SR_CT32_SYNC() __builtin_amdgcn_wave_barrier()
#else
#define SR_CT32_SYNC() __syncthreads()
#endif

// One half-length transform: the thread's N1 inputs v[] (natural order, element tid + 256 n1) -> for the 16 N1 threads
// (k1, k2a) = (tid >> 4, tid & 15), k1 < N1: w[p] = X[k1 + N1 (k2a + 16 rev4(p))].  The caller has made sure nobody still
// reads the LDS image; on return every thread has read what it needs from it (row tid is the thread's own).
// SPECTRUM: the forward transforms of the loop -- the half of the row a partner thread reads (frequencies k2b >= 8: the partner
// of (k, k2b' < 8) sits at 15 - k2b'; thread 0 pairs k2b' with 16 - k2b': 9 .. 15 and the pad slot, where it leaves Z[0]) goes
// back to the thread's own row in frequency order, INSIDE the block that computed it: behind the block all 16 values would be live
// at once across a branch merge (10 registers over the budget of four waves per SIMD, spilled and reloaded every pass).
template <int N1, bool SPECTRUM>
__device__ __forceinline__ void rfft32_workgroup(c32 *v, c32 *w, c32 *lds, const c32 *tw1, int tid
#ifdef SR_CT32_STAMPS
                                                 , long long *stamp_acc, long long &stamp_t
#endif
)
{
    FStage1<N1>::run(v);
    applyf_twiddles<N1, FStage1<N1>>(v, tw1, tid);
    {
        c32 *b = lds + tid + (tid >> 4);                          // element k1*256 + tid, one pad slot per 16
#pragma unroll
        for (int p = 0; p < N1; ++p) b[272 * FStage1<N1>::k1(p)] = v[p];
    }
    SR_STAMP(0)
    SR_CT32_SYNC();
    SR_STAMP(1)
    const int k1 = tid >> 4, lo = tid & 15;
    const bool act = k1 < N1;
    if (act) {
        c32 u[16];
        const c32 *b = lds + 272 * k1 + lo;                       // element k1*256 + lo + 16 h -> + 17 h
#pragma unroll
        for (int h = 0; h < 16; ++h) u[h] = b[17 * h];
#ifdef SR_CT32_STAMPS
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        SR_STAMP(2)
#endif
        fftf_reg<4>(u);
        {
            const c32 *tw = lds + rfft_img_slots(N1) + lo;         // w_256^(lo k2a) at [k2a*16 + lo], filled at kernel start
#pragma unroll
            for (int p = 1; p < 15; p += 2) cmulf2(u[p], tw[16 * bitrev<4>(p)], u[p + 1], tw[16 * bitrev<4>(p + 1)]);
            u[15] = cmulf(u[15], tw[16 * bitrev<4>(15)]);
        }
        // in place (see k_ct_rfft): the cells this thread has read are the ones it writes
        c32 *bw = lds + 272 * k1 + lo;
#pragma unroll
        for (int p = 0; p < 16; ++p) bw[17 * bitrev<4>(p)] = u[p];
        SR_STAMP(3)
    }
    // row tid was written by the thread's own 16-lane group, and the LDS operations of one wave complete in order: only the
    // compiler must not move the reads above the writes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (act) {
        const c32 *b = lds + 17 * tid;
#pragma unroll
        for (int e = 0; e < 16; ++e) w[e] = b[e];
#ifdef SR_CT32_STAMPS
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        SR_STAMP(4)
#endif
        fftf_reg<4>(w);
        SR_STAMP(5)
        if (SPECTRUM) {
            c32 *bo = lds + 17 * tid;
#pragma unroll
            for (int p = 0; p < 16; ++p)
                if (bitrev<4>(p) >= 8) bo[bitrev<4>(p)] = w[p];
            if (tid == 0) bo[16] = w[0];
        }
    }
}

constexpr float kUnitTolF = 5e-7f;

// planes of signal c (0 = x, 1 = y, 2 = z): c = 1, 2: x y;  3: x z;  4: y z;  5 (|u|^2): x y, then z
__device__ __forceinline__ int f32_plane_a(int c) { return c == 4 ? 1 : 0; }
__device__ __forceinline__ int f32_plane_b(int c) { return c == 3 || c == 4 ? 2 : 1; }

// The transforms' inputs.  The epilogue forms them a second time for e[j] and relies on getting the SAME bits: one definition.
SR_PK c32 f32_sig0(c32 x, c32 y, c32 z, float m) { return pk_fma(z + z, z, -pk_fma(x, x, pk_fma(y, y, splat(m)))); }   // 2 z^2 - x^2 - y^2 - m
SR_PK c32 f32_sig1(c32 x, c32 y, float m) { return pk_fma(x, x, -pk_fma(y, y, splat(m))); }                            // x^2 - y^2 - m
SR_PK c32 f32_sigp(c32 a, c32 b, float m) { return pk_fma(a, b, splat(-m)); }                                          // a b - m
SR_PK c32 f32_sig5(c32 x, c32 y, c32 z, float m) { return pk_fma(z, z, pk_fma(x, x, pk_fma(y, y, splat(-m)))); }       // |u|^2 - m

}  // namespace
