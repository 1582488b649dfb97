// sr_ct_rfft64.hip -- kernel 1 with REAL-input float64 transforms (k_ct_rfft), M = 6144 / 8192 points: the float64 kernel of
// 4096 < F + L <= 8192 (option "ct_fft" = 2; the dispatch of sr_ct.hip), and the layout k_ct_rfft32 (sr_ct32.hip) follows.
//
// Reference semantics: calculate_Ct_Palmer, calculate-Ct-from-traj.py:200-238 (see include/spinrelax_hip.h).
//
// Same mathematics as k_ct_fft (six autocorrelations by Wiener-Khinchin, float64), restructured around occupancy: the six
// signals are real, so each goes through a complex transform of HALF the padded length (z[m] = a[2m] + i a[2m+1],
// H = M/2 points) and the real even power spectrum comes back through ONE half-length transform.  The LDS image of a
// transform shrinks from 96 KB to 52 KB (H = 3072): THREE workgroups share a CU's 160 KB instead of one, at <= 168
// registers per lane -- k_ct_fft runs at one wave per SIMD (256 VGPR + 196 AGPR) and is latency-bound.  Seven half-length
// transforms per series replace four full-length ones (20 % fewer flop).
//
// H = N1 * 256 (N1 = 12: M = 6144, the F = 4096 chunks; N1 = 16: M = 8192), 256 threads, three steps N1 x 16 x 16 with
// every small transform in registers:
//   1. thread n2 holds z[n2 + 256 n1], n1 < N1: N1-point transform (12 = 3 x 4), twiddle w_H^(n2 k1), to LDS as
//      element k1*256 + n2 (one pad slot per 16);
//   2. thread (k1, lo), k1 < N1 (16 N1 of the 256 threads): 16-point transform over h (n2 = lo + 16 h), twiddle
//      w_256^(lo k2a), to LDS row (k1*16 + k2a), column lo (rows of 17 slots);
//   3. thread (k1, k2a): reads its own row, 16-point transform over lo: X[k1 + N1 (k2a + 16 k2b)], k2b < 16.
// Real-signal spectrum from Z = FFT_H(z):  A[k] = (Z[k] + conj Z[H-k])/2 - (i/2) w_M^k (Z[k] - conj Z[H-k]); the partner
// frequency H - k lives in thread (N1-k1, 15-k2a) at 15-k2b (k1 = 0 apart), fetched through the row layout.
// Back: with P[k] the weighted power spectrum (P[M-k] = P[k]),  Y[k] = (P[k] + P[H-k]) + i (P[k] - P[H-k]) conj(w_M^k);
// FFT_H(Y)[m] = M (S[2m] + i S[2m-1]): the even lags in the real part, the odd ones in the imaginary part.
// All LDS accesses are 16-byte (one complex) and conflict-free for the lane groups of ds_read_b128 / ds_write_b128
// (MI355X_MICROARCH.md, LDS) except a 2-way case in the natural-order read of Y.
#include "sr_fft64.h"

namespace {

// instead of N (the sequential chain cost 12 % of the kernel: every wave waits on it at one or two waves per SIMD)
template <int N, class KOF>
__device__ __forceinline__ void apply_twiddles_tree(cplx *v, cplx base)
{
    cplx pw[N];
    pw[1] = base;
#pragma unroll
    for (int k = 2; k < N; ++k) pw[k] = cmul(pw[k >> 1], pw[k - (k >> 1)]);
#pragma unroll
    for (int p = 0; p < N; ++p) {
        const int k = KOF::k1(p);
        if (k != 0) v[p] = cmul(v[p], pw[k]);
    }
}

// Where the members of Ct64Tab::Rfft start, in complex entries.  (With the argument typed as the struct and the members named
// in the kernel, the addresses come out of other instructions and k_ct_rfft -- at its register limit -- compiles differently: tried.)
constexpr int kRfftWH = offsetof(Ct64Tab::Rfft, wH) / 16, kRfftW256 = offsetof(Ct64Tab::Rfft, w256) / 16, kRfftWM = offsetof(Ct64Tab::Rfft, wM) / 16;
struct CtRfftArgs {
    const float *soa;
    int64_t Npad;
    const int64_t *chunk_start;   // device, may be null
    const double *tab;            // the Ct64Tab::Rfft of the kernel's N1, read as complex entries kRfftWH / kRfftW256 / kRfftWM + t
    double *psum;                 // (nV, R, Lp)
    int R, F, L, Lp;
};

// One half-length transform: the thread's N1 inputs v[] (natural order, element tid + 256 n1) -> for the 16 N1 threads
// (k1, k2a) = (tid >> 4, tid & 15), k1 < N1: w[p] = X[k1 + N1 (k2a + 16 rev4(p))].  The caller has made sure nobody still
// reads the LDS image; on return every thread has read what it needs from it (row tid is the thread's own).
template <int N1>
__device__ __forceinline__ void rfft_workgroup(cplx *v, cplx *w, cplx *lds, cplx base1, int tid)
{
    RStage1<N1>::run(v);
    apply_twiddles_tree<N1, RStage1<N1>>(v, base1);
    {
        cplx *b = lds + tid + (tid >> 4);                         // element k1*256 + tid, one pad slot per 16
#pragma unroll
        for (int p = 0; p < N1; ++p) b[272 * RStage1<N1>::k1(p)] = v[p];
    }
    __syncthreads();
    const int k1 = tid >> 4, lo = tid & 15;
    const bool act = k1 < N1;
    cplx u[16];
    if (act) {
        const cplx *b = lds + 272 * k1 + lo;                      // element k1*256 + lo + 16 h -> + 17 h
#pragma unroll
        for (int h = 0; h < 16; ++h) u[h] = b[17 * h];
        fft_reg<4>(u);
        {
            const cplx *tw = lds + rfft_img_slots(N1) + lo;       // w_256^(lo k2a) at [k2a*16 + lo], filled at kernel start
#pragma unroll
            for (int p = 1; p < 16; ++p) u[p] = cmul(u[p], tw[16 * bitrev<4>(p)]);
        }
        // in place: element k1*256 + lo + 16 h sits in row (k1*16 + h), column lo -- the very cells this thread has just
        // read are the ones it writes as row (k1*16 + k2a), column lo: no barrier between its reads and its writes
        cplx *bw = lds + 272 * k1 + lo;
#pragma unroll
        for (int p = 0; p < 16; ++p) bw[17 * bitrev<4>(p)] = u[p];
    }
    // The row thread tid reads next (17 tid .. 17 tid + 15) was written by the 16 threads (k1, lo = 0..15) = 16 k1 .. 16 k1 + 15:
    // its own 16-lane group.  LDS operations of one wave complete in order, so no workgroup barrier is needed here -- only
    // the compiler must not move the reads above the writes.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (act) {
        const cplx *b = lds + 17 * tid;
#pragma unroll
        for (int e = 0; e < 16; ++e) w[e] = b[e];
        fft_reg<4>(w);
    }
}

// HALF: the chunk fills at most 2/3 (N1 = 12) or 1/2 (N1 = 16) of the padded length: the thread's inputs beyond NZ are
// known to be zero and are neither loaded nor multiplied.
//
// TR ("traceless"): FIVE forward transforms instead of six.  With T = u (x) u and s = |u|^2,
//     (u.u')^2 = sum_ij T_ij T'_ij = sum_ij Q_ij Q'_ij + s s' / 3,        Q = T - (s/3) 1   (traceless, 5 components),
//     sum_ij Q_ij Q'_ij = d1 d1'/2 + d2 d2'/6 + 2 (xy x'y' + xz x'z' + yz y'z'),  d1 = x^2 - y^2,  d2 = 2 z^2 - x^2 - y^2
// (an orthonormal change of basis on the diagonal (x^2, y^2, z^2); exact for ANY vectors).  The bond vectors are unit
// vectors rounded to float32: s = 1 + e with |e| < 3e-7, so the trace term needs no transform,
//     sum_{j < F-d} s_j s_{j+d} = (F - d) + P[F-d] + (P[F] - P[d]) + O(F e^2),      P[k] = sum_{j<k} e_j  (prefix sums),
// and the neglected O(e^2) part is < 1e-13 of C(t).  P[F-d] + (P[F] - P[d]) = G[0] + G[d] with G[d] = sum_{j=d}^{F-d-1} e_j, the
// sum over a window that shrinks from both ends: a suffix scan over HALF the series.  The prologue (which holds x, y, z for the
// first signal anyway) forms e, the workgroup scans it once in float32 with DPP adds, and the finished term
// ((F - d) + G[0] + G[d]) / 3 stays in LDS as float64 (16 KB) until the lags are written: one look-up and one fma per lag.
// Measured (rocprofv3 PMC, cfg3): 7.1 % fewer VALU instructions per launch than the six-signal kernel (a seventh of the
// transforms minus this bookkeeping), 3.4 % fewer wave cycles, 0.95 -> 0.915 ms: the kernel's waves spend 36 % of their life
// at barriers / waitcnt and 22 % in issue stalls, which a shorter instruction stream does not shorten.  (The first version --
// float64 prefix sums over the whole series through ds_bpermute shuffles, three look-ups per lag -- cost as much as it saved.)
// A series with any |e| >= kUnitTol (not a unit vector: zero vectors from the 0/0 guard of vecnorm_NDarray, callers with
// unnormalised input) runs the sixth transform on s instead -- decided per workgroup, same kernel.
constexpr double kUnitTol = 5e-7;

template <bool TR> __device__ __forceinline__ int rfft_plane_a(int c) { return TR ? (c == 4 ? 1 : 0) : (c < 3 ? c : (c == 5 ? 1 : 0)); }
template <bool TR> __device__ __forceinline__ int rfft_plane_b(int c) { return TR ? (c == 3 || c == 4 ? 2 : 1) : (c < 3 ? c : (c == 3 ? 1 : 2)); }
// weight / 4 of signal c in the power spectrum
template <bool TR> __device__ __forceinline__ double rfft_weight4(int c)
{
    if (!TR) return c < 3 ? 0.25 : 0.5;
    return c == 0 ? 1.0 / 24.0 : (c == 1 ? 0.125 : (c == 5 ? 1.0 / 12.0 : 0.5));
}

// (A register budget below the 256 that two waves per SIMD allow -- amdgpu_num_vgpr, which counts in units of TWO registers on
// gfx90a and later -- was tried to leave the bandwidth kernels room beside a C(t) + fit pair of waves: 240 / 232 / 224 VGPRs
// cost 36-52 B of scratch in the transform loop, 0.93 -> 1.01 / 1.01 / 1.10 ms alone, no hiding gained)
template <int N1, bool HALF, bool TR>
__global__ __launch_bounds__(256, 2) void k_ct_rfft(CtRfftArgs a)
{
    extern __shared__ __align__(16) unsigned char fft_smem[];
    cplx *lds = reinterpret_cast<cplx *>(fft_smem);
    constexpr int H = N1 * 256, M = 2 * H;
    constexpr int NZ = HALF ? (N1 == 12 ? 8 : N1 / 2) : N1;
    // PF: the samples of signal c + 1 are loaded one transform ahead (2 NZ float2 registers held across the transform).  With
    // all 16 input blocks in use that is 64 VGPRs the 256-register budget does not have (188 B of scratch, reloaded inside the
    // transform): the M = 8192 kernel loads them right before it forms the signal and leaves the latency to the other
    // workgroup of the CU.
    constexpr bool PF = NZ <= 8;
    float *Pl = reinterpret_cast<float *>(lds + rfft_img_slots(N1) + 512);     // TR: the trace term's table (2049 doubles), then scan scratch
    const int tid0 = threadIdx.x;
    const int v = blockIdx.x / a.R, r = blockIdx.x - v * a.R;
    const int F = a.F;
    const int64_t start = a.chunk_start ? a.chunk_start[r] : (int64_t)r * F;
    const float *px = a.soa + ((int64_t)v * 3 + 0) * a.Npad + start;
    const bool even = ((start | a.Npad | (int64_t)F) & 1) == 0;   // frames 2m, 2m + 1 of every plane share an aligned 8 bytes,
                                                                  // and no pair straddles the end of the chunk
    // partner thread holding the frequencies H - k (see the header comment): pt; thread 0 pairs k2b with (16 - k2b) & 15,
    // everybody else with 15 - k2b: column (15 - k2b + off0) & 15, which only wraps for thread 0 at k2b = 0
    const cplx wbase = {a.tab[2 * (kRfftWM + ((tid0 >> 4) < N1 ? (tid0 >> 4) + N1 * (tid0 & 15) : 0))],
                        a.tab[2 * (kRfftWM + ((tid0 >> 4) < N1 ? (tid0 >> 4) + N1 * (tid0 & 15) : 0)) + 1]};   // w_M^(k1 + N1 k2a)

    // Power spectrum, by PAIRS of frequencies (k, H - k): thread (k1, k2a) owns the pairs whose k has k2b < 8; it keeps
    // Wk[q] = P[k] (k2b = q) and Wm[q] = P[H - k] (the partner thread's frequency 15 - q).  With S = Z[k] + conj Z[H-k],
    // D = Z[k] - conj Z[H-k], T = w_M^k D:   4 |A[k]|^2 = |S - i T|^2   and   4 |A[H-k]|^2 = |S + i T|^2  -- one complex
    // multiply serves both.  Thread 0 is its own partner with k2b <-> 16 - k2b: its slot q = 0 holds k = 0 (Wk) and k = H
    // (Wm), and the self-paired frequency k = H/2 (k2b = 8) gets the scalar Wmid.
    double Wk[8], Wm[8], Wmid = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) Wk[q] = Wm[q] = 0.0;

    // signal c is a product of two of the three planes (TR: c = 1 is x^2 - y^2; c = 0 and 5 need all three, see below).
    // Thread t holds the pairs of frames (2m, 2m + 1), m = t + 256 n1; unconditional range-checked loads (no branch per
    // sample), one 8-byte load per plane when the pair is aligned.  The loads of signal c + 2 are issued right after the
    // samples of signal c + 1 have been turned into its input, i.e. a whole transform before they are needed (15 % of the
    // kernel was spent waiting for them at the top of every transform).
    // Loads go through buffer resources that cover exactly the chunk's F frames of a plane: a frame past the chunk reads
    // as 0 by the hardware range check -- no clamp, no select, and the address is one 32-bit byte offset per load instead
    // of a 64-bit add (13 % of the transform loop's instructions were address arithmetic and masks).
    float2 ar[NZ], br[NZ];
#define SR_RFFT_LOAD1(DST, PLANE, T)                                                             \
    {                                                                                            \
        /* the plane index is workgroup-uniform: say so, or the descriptor is built in VGPRs and every load becomes a */ \
        /* waterfall loop (readfirstlane + compare + masked load), 13 instructions and a serialisation each          */ \
        const __amdgpu_buffer_rsrc_t rs_ = __builtin_amdgcn_make_buffer_rsrc(                    \
            const_cast<float *>(px + (int64_t)__builtin_amdgcn_readfirstlane(PLANE) * a.Npad), (short)0, F * 4, 0x00020000); \
        if (even) {                                                                              \
            _Pragma("unroll") for (int n1 = 0; n1 < NZ; ++n1)                                    \
                DST[n1] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rs_, 8 * ((T) + 256 * n1), 0, 0)); \
        } else {                                                                                 \
            _Pragma("unroll") for (int n1 = 0; n1 < NZ; ++n1) {                                  \
                const int ob_ = 8 * ((T) + 256 * n1);                                            \
                DST[n1] = make_float2(__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_, ob_, 0, 0)),      \
                                      __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_, ob_ + 4, 0, 0))); \
            }                                                                                    \
        }                                                                                        \
    }
#define SR_RFFT_LOAD(C, T)                                                                       \
    {                                                                                            \
        const int cc_ = (C);                                                                     \
        SR_RFFT_LOAD1(ar, rfft_plane_a<TR>(cc_), T)                                              \
        SR_RFFT_LOAD1(br, rfft_plane_b<TR>(cc_), T)                                              \
    }
    {
        // step-2 twiddles w_256^(lo k2a), transposed so that the 16 lanes of a ds_read_b128 group (consecutive lo) hit 16
        // consecutive slots; ordered before their first use by the first barrier of the first transform
        const int j = ((tid0 & 15) * (tid0 >> 4)) & 255;
        lds[rfft_img_slots(N1) + tid0] = cplx{a.tab[2 * (kRfftW256 + j)], a.tab[2 * (kRfftW256 + j) + 1]};
    }

    // step-1 twiddle base w_H^tid: the same for every transform of the series.  From a table in LDS, not from global
    // memory: vmcnt counts in order, so waiting for a global load issued behind the sample prefetch drains the prefetch too
    // (measured: 0.94 -> 1.00 ms although a seventh of the transforms was gone), and carrying it in registers across the
    // transforms costs four of the VGPRs the loop does not have.  Ordered before its first read by the first barrier below.
    lds[rfft_img_slots(N1) + 256 + tid0] = cplx{a.tab[2 * (kRfftWH + tid0)], a.tab[2 * (kRfftWH + tid0) + 1]};
    cplx sig[N1];                 // input of the next transform (entries >= NZ stay zero)
#pragma unroll
    for (int n1 = 0; n1 < N1; ++n1) sig[n1] = cplx{0.0, 0.0};
    int nsig = 6;
    if (TR) {
        // ---- prologue of the traceless form: signal 0 = 2 z^2 - x^2 - y^2, and the trace term's table ----
        // e_j = |u_j|^2 - 1 (float64, then rounded to float32: |e| < 3e-7, so 1e-14 absolute).  What the lags need is
        //     P[F-d] + (P[F] - P[d]) = G[0] + G[d],      G[d] = sum_{j = d}^{F-d-1} e_j  (the window that shrinks from both ends),
        // and G is a suffix sum of h_i = e_i + e_{F-1-i} (i < F-1-i; the centre frame once): a scan over HALF the series,
        // in float32 (sums of < 4096 terms of 1e-7: rounding 1e-12 absolute against F - d > 2000), with DPP adds.
        float emax = 0.f;
        float *E = reinterpret_cast<float *>(lds);          // scratch in the still unused transform image
        float *aux = Pl + 2 * 2056;                         // behind the table: [0 .. 4) wave totals, [4 .. 8) wave maxima of |e|
        {
            float2 zr[NZ];
            SR_RFFT_LOAD(0, tid0)                      // x, y
            SR_RFFT_LOAD1(zr, 2, tid0)
            const bool full = F == 512 * NZ;           // no frame of the loaded blocks lies behind the chunk
#pragma unroll
            for (int n1 = 0; n1 < NZ; ++n1) {
                const double x0 = (double)ar[n1].x, x1 = (double)ar[n1].y, y0 = (double)br[n1].x, y1 = (double)br[n1].y;
                const double z0 = (double)zr[n1].x, z1 = (double)zr[n1].y;
                const double q0 = fma(x0, x0, y0 * y0), q1 = fma(x1, x1, y1 * y1), zz0 = z0 * z0, zz1 = z1 * z1;
                sig[n1] = cplx{(zz0 + zz0) - q0, (zz1 + zz1) - q1};
                const int f0 = 2 * (tid0 + 256 * n1);
                float ea = (float)((q0 + zz0) - 1.0), eb = (float)((q1 + zz1) - 1.0);
                if (!full) {
                    ea = f0 < F ? ea : 0.f;
                    eb = f0 + 1 < F ? eb : 0.f;
                }
                *reinterpret_cast<float2 *>(E + f0) = make_float2(ea, eb);
                emax = fmaxf(emax, fmaxf(fabsf(ea), fabsf(eb)));
            }
        }
        SR_RFFT_LOAD(1, tid0)
        const int lane = tid0 & 63, wave = tid0 >> 6;
        emax = wave_max_f32(emax);                           // |e| >= 0, so 0 is neutral
        if (lane == 63) aux[4 + wave] = emax;
        __syncthreads();
        // thread t owns i = 8 b .. 8 b + 7 with b = 255 - t: an inclusive PREFIX scan over t is the suffix sum over i
        const int i0 = 8 * (255 - tid0);
        float sfx[8], incl;
        {
            const float4 ea = *reinterpret_cast<const float4 *>(E + i0), eb = *reinterpret_cast<const float4 *>(E + i0 + 4);
            const float ei[8] = {ea.x, ea.y, ea.z, ea.w, eb.x, eb.y, eb.z, eb.w};
            float h[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int i = i0 + k, j = F - 1 - i;               // j > 0: F > 2730 for this transform length
                const float ej = E[j];
                h[k] = i < j ? ei[k] + ej : (i == j ? ei[k] : 0.f);
            }
            sfx[7] = h[7];
#pragma unroll
            for (int k = 6; k >= 0; --k) sfx[k] = h[k] + sfx[k + 1];
            incl = wave_scan_f32(sfx[0]);                    // wave-wide inclusive scan of the thread totals
            if (lane == 63) aux[wave] = incl;
        }
        __syncthreads();                                     // every read of E is done: the first transform may use the image
        {
            float off = incl - sfx[0];
#pragma unroll
            for (int w2 = 0; w2 < 3; ++w2) off += w2 < wave ? aux[w2] : 0.f;
            const float G0 = (aux[0] + aux[1]) + (aux[2] + aux[3]);          // sum of every e of the series
            // Tt[d] = ((F - d) + G[0] + G[d]) / 3: the finished trace term of lag d, float64 -- one fma per lag at the end
            double *Tt = reinterpret_cast<double *>(Pl);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                Tt[i0 + k] = ((double)(F - (i0 + k)) + (double)(G0 + (sfx[k] + off))) * (1.0 / 3.0);
            if (tid0 == 0) Tt[2048] = ((double)(F - 2048) + (double)G0) * (1.0 / 3.0);
            const float mx = fmaxf(fmaxf(aux[4], aux[5]), fmaxf(aux[6], aux[7]));
            nsig = __builtin_amdgcn_readfirstlane(mx < (float)kUnitTol ? 5 : 6);
        }
    } else {
        SR_RFFT_LOAD(0, tid0)
#pragma unroll
        for (int n1 = 0; n1 < NZ; ++n1)
            sig[n1] = cplx{(double)ar[n1].x * (double)br[n1].x, (double)ar[n1].y * (double)br[n1].y};
        if (PF) SR_RFFT_LOAD(1, tid0)
    }
#pragma unroll 1
    for (int c = 0; c < nsig; ++c) {
        asm volatile("" ::: "memory");
        const int tid = opaque(tid0);
        const int k1 = tid >> 4, k2a = tid & 15;
        const bool act = k1 < N1;
        const int pt = k1 != 0 ? (N1 - k1) * 16 + (15 - k2a) : (k2a != 0 ? 16 - k2a : 0);
        const int off0 = tid == 0 ? 1 : 0;
        const cplx base1 = opaque(lds[rfft_img_slots(N1) + 256 + tid]);
        cplx w[16];
        rfft_workgroup<N1>(sig, w, lds, base1, tid);
        // own row again, now in frequency order k2b; then every thread reads the partner frequencies of its 8 pairs
        if (act) {
            cplx *b = lds + 17 * tid;
#pragma unroll
            for (int p = 0; p < 16; ++p) b[bitrev<4>(p)] = w[p];
        }
        __syncthreads();
        if (act) {
            const double wgt = rfft_weight4<TR>(c);               // weight / 4
            const cplx *b = lds + 17 * pt + off0;
            const cplx wb = opaque(wbase);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const cplx zk = w[bitrev<4>(q)];
                if (q == 0 && off0) {                              // thread 0: k = 0 and k = H from Z[0] alone
                    const double e0 = zk.re + zk.im, eh = zk.re - zk.im;
                    Wk[0] = fma(4.0 * wgt, e0 * e0, Wk[0]);
                    Wm[0] = fma(4.0 * wgt, eh * eh, Wm[0]);
                    continue;
                }
                const cplx zm = b[15 - q];
                const cplx S = {zk.re + zm.re, zk.im - zm.im}, D = {zk.re - zm.re, zk.im + zm.im};
                const cplx T = cmul(mul_w32_rt(wb, q), D);
                const double pr = S.re + T.im, pi = S.im - T.re;      // S - i T
                const double mr = S.re - T.im, mi = S.im + T.re;      // S + i T
                Wk[q] = fma(wgt, fma(pr, pr, pi * pi), Wk[q]);
                Wm[q] = fma(wgt, fma(mr, mr, mi * mi), Wm[q]);
            }
            if (off0) {                                            // k = H/2 (k2b = 8) mirrors onto itself
                const cplx zk = w[bitrev<4>(8)];
                const cplx S = {2.0 * zk.re, 0.0}, D = {0.0, 2.0 * zk.im};
                const cplx T = cmul(mul_w32_rt(wb, 8), D);
                const double pr = S.re + T.im, pi = S.im - T.re;
                Wmid = fma(wgt, fma(pr, pr, pi * pi), Wmid);
            }
        }
        // the next signal's input from the samples loaded one transform ago (w is dead here: few live registers), and the loads
        // of the one after it.  Unconditional (behind the last signal the values are simply not used): a conditional
        // assignment would keep the transform's in-place leftovers in `sig` alive through the spectrum step.
        {
            const int cn = c + 1;
            if (!PF && cn < nsig) SR_RFFT_LOAD(cn, tid)
            // keep these products HERE: nothing ties them to this point but their inputs, and scheduled above the spectrum
            // step (where w[16] is live) they push the accumulators into scratch
#pragma unroll
            for (int n1 = 0; n1 < NZ; ++n1)
                asm volatile("" : "+v"(ar[n1].x), "+v"(ar[n1].y), "+v"(br[n1].x), "+v"(br[n1].y));
#pragma unroll
            for (int n1 = NZ; n1 < N1; ++n1) sig[n1] = cplx{0.0, 0.0};
            if (TR && cn == 1) {                                   // x^2 - y^2
#pragma unroll
                for (int n1 = 0; n1 < NZ; ++n1) {
                    const double a0 = (double)ar[n1].x, a1 = (double)ar[n1].y, b0 = (double)br[n1].x, b1 = (double)br[n1].y;
                    sig[n1] = cplx{fma(a0, a0, -(b0 * b0)), fma(a1, a1, -(b1 * b1))};
                }
            } else {
#pragma unroll
                for (int n1 = 0; n1 < NZ; ++n1)
                    sig[n1] = cplx{(double)ar[n1].x * (double)br[n1].x, (double)ar[n1].y * (double)br[n1].y};
            }
            if (TR && cn == 5 && nsig == 6) {          // not a unit vector: s = x^2 + y^2 + z^2 itself (rare; the z load is exposed)
#pragma unroll
                for (int n1 = 0; n1 < NZ; ++n1) {
                    const double a0 = (double)ar[n1].x, a1 = (double)ar[n1].y, b0 = (double)br[n1].x, b1 = (double)br[n1].y;
                    sig[n1] = cplx{fma(a0, a0, b0 * b0), fma(a1, a1, b1 * b1)};
                }
                SR_RFFT_LOAD1(ar, 2, tid)
#pragma unroll
                for (int n1 = 0; n1 < NZ; ++n1) {
                    const double z0 = (double)ar[n1].x, z1 = (double)ar[n1].y;
                    sig[n1] = cplx{fma(z0, z0, sig[n1].re), fma(z1, z1, sig[n1].im)};
                }
            } else if (PF && c + 2 < nsig) {
                SR_RFFT_LOAD(c + 2, tid)
            }
        }
        __syncthreads();
    }

    // ---- back: Y[k] = (P[k] + P[H-k]) + i (P[k] - P[H-k]) conj(w_M^k), through the same transform.  The pair owner has
    // both P[k] and P[H-k]:  Y[k] = (E - d sin, d cos),  Y[H-k] = (E + d sin, d cos)  with E = P[k] + P[H-k],
    // d = P[k] - P[H-k], w_M^k = (cos, -sin).  Natural order with one pad slot per N1 elements: k + k2a + 16 k2b. ----
    const int tid = opaque(tid0);
    const int k1 = tid >> 4, k2a = tid & 15;
    const bool act = k1 < N1;
    const int pt = k1 != 0 ? (N1 - k1) * 16 + (15 - k2a) : (k2a != 0 ? 16 - k2a : 0);
    const int off0 = tid == 0 ? 1 : 0;
    if (act) {
        cplx *bk = lds + k1 + (N1 + 1) * k2a;                                    // own frequencies, column k2b = q
        cplx *bm = lds + (pt >> 4) + (N1 + 1) * (pt & 15) + 16 * (N1 + 1) * off0;  // the partner's, column 15 - q (+ 1 for thread 0)
        const cplx wb = opaque(wbase);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const double E = Wk[q] + Wm[q], d = Wk[q] - Wm[q];
            const cplx wk = mul_w32_rt(wb, q);                                  // (cos, -sin)
            bk[16 * (N1 + 1) * q] = {fma(d, wk.im, E), d * wk.re};
            if (!(q == 0 && off0)) bm[16 * (N1 + 1) * (15 - q)] = {fma(-d, wk.im, E), d * wk.re};
        }
        if (off0) bk[16 * (N1 + 1) * 8] = {2.0 * Wmid, 0.0};                     // k = H/2: E = 2 P, d = 0
    }
    __syncthreads();
    {
        cplx yin[N1];
#pragma unroll
        for (int n1 = 0; n1 < N1; ++n1) {
            const int k = tid + 256 * n1;
            yin[n1] = lds[k + k / N1];
        }
        __syncthreads();
        cplx w[16];
        rfft_workgroup<N1>(yin, w, lds, opaque(lds[rfft_img_slots(N1) + 256 + tid]), tid);
        if (act) {
            double *out = a.psum + ((int64_t)v * a.R + r) * a.Lp;
            const double inv = 1.0 / (double)M;
            const bool unit = TR && nsig == 5;
            const double *Tt = reinterpret_cast<const double *>(Pl);
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const int m = k1 + N1 * (k2a + 16 * bitrev<4>(p));
                const int le = 2 * m, lod = 2 * m - 1;
                if (le >= 1 && le <= a.L) out[le] = unit ? fma(w[p].re, inv, Tt[le]) : w[p].re * inv;
                if (lod >= 1 && lod <= a.L) out[lod] = unit ? fma(w[p].im, inv, Tt[lod]) : w[p].im * inv;
            }
        }
    }
#undef SR_RFFT_LOAD
#undef SR_RFFT_LOAD1
}

template <int N1, bool HALF, bool TR>
constexpr size_t rfft_lds_bytes()
{
    // transform image + the 16 x 16 step-2 twiddles + the 256 step-1 twiddle bases (+ TR: the trace term's table Tt[0 .. 2048]
    // as float64, then 4 wave totals and 4 wave maxima)
    return (size_t)(rfft_img_slots(N1) + 512) * sizeof(cplx) + (TR ? (size_t)(2 * 2056 + 16) * sizeof(float) : 0);
}

template <int N1, bool HALF, bool TR>
int launch_ct_rfft_h(sr_ctx *ctx, const CtRfftArgs &a, int64_t series)
{
    return sr_launch(ctx, k_ct_rfft<N1, HALF, TR>, dim3((unsigned)series), dim3(256), rfft_lds_bytes<N1, HALF, TR>(), a);
}
// With L = F/2 the two transform lengths are tied to the chunk length: M = 6144 serves 4096 < 1.5 F <= 6144, i.e. F <= 4096
// (at most 8 of the 12 input blocks are non-zero: HALF), M = 8192 serves 4096 < F <= 5461 (more than half: not HALF).
// Only those instantiations exist.  The traceless form of the M = 6144 kernel is an OPTION (sr_set_option "ct_traceless"):
// alone it is 4 % faster (0.95 -> 0.915 ms for cfg3), inside the pipeline -- where a C(t) workgroup shares its CU with a
// fit workgroup -- 3 % slower per step (same-box A/B), so the six-signal kernel stays the default.
int launch_ct_rfft(sr_ctx *ctx, const CtRfftArgs &a, int64_t series)
{
    if (a.F + a.L <= 6144) {
        SR_REQUIRE(a.F <= 4096, -3, "k_ct_rfft<12>: F=%d does not fit 8 input blocks", a.F);
        return ctx->ct_traceless ? launch_ct_rfft_h<12, true, true>(ctx, a, series) : launch_ct_rfft_h<12, true, false>(ctx, a, series);
    }
    SR_REQUIRE(a.F + a.L <= 8192, -3, "k_ct_rfft<16>: F=%d too long", a.F);
    return launch_ct_rfft_h<16, false, false>(ctx, a, series);
}

}  // namespace

// Called by sr_ct_palmer_sums_f32_dev (sr_ct.hip): half-length transforms, two workgroups per CU.
int sr_launch_ct_rfft64(sr_ctx *ctx, const sr_ct_job &j)
{
    CtRfftArgs a;
    a.soa = j.soa; a.Npad = j.Npad; a.chunk_start = j.cs_dev; a.psum = j.psum;
    a.R = j.R; a.F = j.F; a.L = j.L; a.Lp = j.Lp;
    const Ct64Tab *tab = (const Ct64Tab *)sr_ct64_table(ctx);
    if (!tab) return -5;
    a.tab = tab->rfft[j.F + j.L <= 6144 ? 0 : 1].wH;
    return launch_ct_rfft(ctx, a, j.series);
}
