// sr_noe_tile.h -- the workgroup body and the finish kernel that the all-pairs dipolar map, its lagged form and the lagged form's split
// into tumbling modes share (k_noe_pairs, k_noe_lagged, k_noe_modes: sr_noe.hip).  What differs between them is a Term:
//     kWindows               frame windows staged: 1 (the frames t), or 2 (the origins t and the frames t + k of a lag k)
//     kSums                  sums per pair
//     quat_given(quat)       whether the quaternion threads fetch (the mode-resolved map rotates by its frame alone when quat is null)
//     matrix(q, R)           what a quaternion thread stores for its frame: 3 rows padded to 4 Reals
//     add<ROT>(A, d, ri, M)  the arithmetic per pair and frame on the pair vectors d[w], the reciprocal distances ri[w] and the
//                            frames' matrices M[w]: the term rotates d itself (noe_rotate), where its sequence has the rotation
//     part_offset(m, n)      where sum m of the pair at row r, column c of the tile, n = r kTile + c, lies in a partial tile
//     part_place(e, m, n)    its inverse: the sum m and the pair n of the value at e
//
// noe_tile_body: one workgroup of 256 threads per (block, lag, frame split s < S, tile pair ti <= tj); a tile is kTile = 32 atoms, a
//   thread owns the 2 x 2 pairs (ty + 16 a, tx + 16 c), ty = tid / 16, tx = tid % 16.  LDS holds, per window, kFB = 16 frames of the 64
//   atoms as float4 (x, y, z, -): a wave reads its i-atoms as 4 broadcast addresses and its j-atoms as 16 consecutive float4 (256
//   contiguous bytes, each read by 4 lanes).  The atoms are gathered from xyz by index while they are staged (192 threads, one (atom,
//   component) each, of every window); 16 more threads per window fetch the frames' quaternions and store the matrices, which every
//   thread then reads as broadcasts.  The next stage is fetched into registers while the current one is worked on.
//   A frame split owns a range of ORIGINS (noe_lag_origins; the map is lag 0): a second window reads up to k frames past that range,
//   never past the block's end.
//   d is the difference of the raw float32 coordinates, taken first and in the lab frame: r and every power of it come from that
//   difference, and only what follows sees the rotation, applied to d.  (Rotating the coordinates first would round relative to a
//   coordinate of several nm what is then compared over 0.2 nm, and r^-6 multiplies that by six.)  Explicit operations, no contraction:
//       d_a  = x_ja - x_ia                               1 rounding each
//       r2   = fma(dz, dz, fma(dy, dy, dx * dx))         3 roundings
//       ri   = v_rsq_f32(r2)                             1 ulp          (Real = double: 1 / sqrt)
//       d'_a = fma(Ma0, dx, fma(Ma1, dy, Ma2 * dz))      M the frame's matrix (noe_rotate, called by the term)
//   and the term's own sequence, in float32 partial sums of at most kFlush = 8 frames, which are then added to float64 registers
//   (mode 0, Real = float), or in float64 directly (mode 1, Real = double).
//   Of a diagonal tile the quarter a = 1, c = 0 lies wholly below the diagonal and is skipped (a uniform branch); the other pairs with
//   i >= j and the pairs of atoms past P are computed on whatever was staged (zeros: r = 0, non-finite) and never written out.
//   S > 1: the workgroup writes a partial tile.  S = 1 (few frames, or so many tile pairs that they fill the chip alone: every large
//   map): it writes its pairs i < j < P into out[b][lag][i (2 P - i - 1) / 2 + j - i - 1][kSums] itself, and the call needs no memory
//   beside its result.
// k_noe_finish: adds the S partial tiles of a (block, lag, tile pair) in the order s = 0 .. S-1 and writes the pairs i < j < P.
// No atomics anywhere: equal input gives bit-equal sums.
#pragma once
#include "sr_internal.h"
#include "sr_noe_host.h"

constexpr int kTile = kNoeTile;             // atoms per tile side (sr_noe_host.h)
constexpr int kFB = 16;                     // frames per LDS stage and window
constexpr int kFlush = 8;                   // mode 0: frames per float32 partial sum
constexpr int kRows = 2 * kTile * 3;        // staged series per frame: (side, atom, component) = 192, one thread each
static_assert(kRows + 2 * kFB <= 256 && kFB % kFlush == 0 && kNoeLagPart % 256 == 0, "stage shape");

// tile pair p = 0 .. nT (nT + 1) / 2 - 1, row-major over ti <= tj
__device__ __forceinline__ void noe_tile_pair(int p, int nT, int &ti, int &tj)
{
    ti = 0;
    while (p >= nT - ti) { p -= nT - ti; ++ti; }
    tj = ti + p;
}

__device__ __forceinline__ float noe_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double noe_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float noe_rsqrt(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ double noe_rsqrt(double x) { return 1.0 / sqrt(x); }

// the head of the arithmetic of a pair and frame: d = x_j - x_i of two staged atoms, |d|^2, d' = M d (rows of M padded to 4)
template <typename Real>
__device__ __forceinline__ void noe_diff(const float4 &xj, const float4 &xi, Real *d)
{
#pragma clang fp contract(off)
    d[0] = (Real)xj.x - (Real)xi.x; d[1] = (Real)xj.y - (Real)xi.y; d[2] = (Real)xj.z - (Real)xi.z;
}
template <typename Real>
__device__ __forceinline__ Real noe_norm2(const Real *d)
{
#pragma clang fp contract(off)
    return noe_fma(d[2], d[2], noe_fma(d[1], d[1], d[0] * d[0]));
}
template <bool ROT, typename Real>
__device__ __forceinline__ void noe_rotate(const Real *M, const Real *d, Real *p)
{
#pragma clang fp contract(off)
    p[0] = d[0]; p[1] = d[1]; p[2] = d[2];
    if (ROT) {
        p[0] = noe_fma(M[0], d[0], noe_fma(M[1], d[1], M[2] * d[2]));
        p[1] = noe_fma(M[4], d[0], noe_fma(M[5], d[1], M[6] * d[2]));
        p[2] = noe_fma(M[8], d[0], noe_fma(M[9], d[1], M[10] * d[2]));
    }
}

template <typename Term, typename Real, bool ROT>
__device__ __forceinline__ void noe_tile_body(const Term &term, const float *xyz, int64_t nAtoms, const int *index,
                                              int P, const double *quat, const int64_t *blk,
                                              const int *lags, int K, int nT, int NP, int S, double *part,
                                              double *res, int64_t npairs)
{
#pragma clang fp contract(off)
    // The second window is written out beside the first, `x[0] ...; if (kW > 1) x[w1] ...`, w1 = kW - 1 keeping the index inside a
    // one-window array.  Not loops over the windows: unrolled later, they turned the fetch of k_noe_lagged into selects and its code
    // into another (250 instructions fewer, docs/EXPERIMENTS.md section 36); as written the compiler sees the former kernels' statements.
    constexpr int kW = Term::kWindows, kM = Term::kSums, w1 = kW - 1;
    static_assert(kW == 1 || kW == 2, "one window, or two a lag apart");
    __shared__ float4 crd[kW][kFB][2 * kTile];         // [0]: the frames t, [1]: the frames t + k
    __shared__ Real rot[kW][kFB][12];
    const int tid = threadIdx.x;
    const int bid = blockIdx.x;
    const int p = bid % NP, s = (bid / NP) % S, kq = (bid / (NP * S)) % K, b = bid / (NP * S * K);
    int ti, tj;
    noe_tile_pair(p, nT, ti, tj);
    // origins [f0, f1) of the block that split s owns at this lag
    const int64_t start = blk[2 * b], len = blk[2 * b + 1], lag = kW > 1 ? lags[kq] : 0;
    int64_t lo, hi;
    noe_lag_origins(len, lag, S, s, lo, hi);
    const int64_t f0 = start + lo, f1 = start + hi;    // f1 + lag <= start + len

    // what this thread fetches of every stage: threads 0 .. 191 one (side, atom, component) of each frame of every window, -1 = an
    // atom past P; the kW kFB threads behind them the quaternion of one frame of one window
    int64_t src = -1;
    if (tid < kRows) {
        const int a = tid / 3, c = tid - 3 * a;
        const int g = (a < kTile ? ti * kTile + a : tj * kTile + a - kTile);
        if (g < P) src = (int64_t)index[g] * 3 + c;
    }
    const int qi = tid - kRows;                        // 0 .. kW kFB - 1 on the quaternion threads
    const int qw = kW > 1 && qi >= kFB ? 1 : 0, qf = qi - qw * kFB;
    float pre[kW][kFB];
    double qpre[4] = {1.0, 0.0, 0.0, 0.0};             // never fetched: the identity
    auto fetch = [&](int64_t fs) {
        if (tid < kRows) {
#pragma unroll
            for (int f = 0; f < kFB; ++f) {
                const bool in = src >= 0 && fs + f < f1;
                pre[0][f] = in ? xyz[(fs + f) * nAtoms * 3 + src] : 0.f;
                if (kW > 1) pre[w1][f] = in ? xyz[(fs + f + lag) * nAtoms * 3 + src] : 0.f;
            }
        } else if (ROT && Term::quat_given(quat) && qi < kW * kFB && fs + qf < f1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) qpre[k] = quat[(fs + qf + (qw ? lag : 0)) * 4 + k];
        }
    };

    const int ty = tid >> 4, tx = tid & 15;
    const bool diag = ti == tj;
    Real acc[2][2][kM];
    double tot[2][2][kM];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int m = 0; m < kM; ++m) { acc[a][c][m] = (Real)0; tot[a][c][m] = 0.0; }
    auto flush = [&]() {
        if (sizeof(Real) == sizeof(double)) return;     // mode 1 accumulates in acc, which is float64
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int m = 0; m < kM; ++m) { tot[a][c][m] += (double)acc[a][c][m]; acc[a][c][m] = (Real)0; }
    };

    if (f0 < f1) fetch(f0);
    for (int64_t fs = f0; fs < f1; fs += kFB) {
        __syncthreads();                                   // the previous stage has been read
        if (tid < kRows) {
            const int a = tid / 3, c = tid - 3 * a;
#pragma unroll
            for (int f = 0; f < kFB; ++f) {
                reinterpret_cast<float *>(&crd[0][f][a])[c] = pre[0][f];
                if (kW > 1) reinterpret_cast<float *>(&crd[w1][f][a])[c] = pre[w1][f];
            }
        } else if (ROT && qi < kW * kFB) {
            term.matrix(qpre, rot[qw][qf]);
        }
        __syncthreads();
        if (fs + kFB < f1) fetch(fs + kFB);                // in flight during the arithmetic below
        const int nf = (int)(f1 - fs < kFB ? f1 - fs : (int64_t)kFB);
        for (int f = 0; f < nf; ++f) {
            float4 xi[kW][2], xj[kW][2];
            xi[0][0] = crd[0][f][ty]; xi[0][1] = crd[0][f][ty + 16];
            xj[0][0] = crd[0][f][kTile + tx]; xj[0][1] = crd[0][f][kTile + tx + 16];
            if (kW > 1) {
                xi[w1][0] = crd[w1][f][ty]; xi[w1][1] = crd[w1][f][ty + 16];
                xj[w1][0] = crd[w1][f][kTile + tx]; xj[w1][1] = crd[w1][f][kTile + tx + 16];
            }
            Real M[kW][12];
            if (ROT) {
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    M[0][k] = rot[0][f][k];
                    if (kW > 1) M[w1][k] = rot[w1][f][k];
                }
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    if (diag && a == 1 && c == 0) continue;
                    Real d[kW][3], r2[kW], ri[kW];
                    noe_diff(xj[0][c], xi[0][a], d[0]);
                    if (kW > 1) noe_diff(xj[w1][c], xi[w1][a], d[w1]);
                    r2[0] = noe_norm2(d[0]);
                    if (kW > 1) r2[w1] = noe_norm2(d[w1]);
                    ri[0] = noe_rsqrt(r2[0]);
                    if (kW > 1) ri[w1] = noe_rsqrt(r2[w1]);
                    Term::template add<ROT>(acc[a][c], d, ri, M);
                }
            if ((f & (kFlush - 1)) == kFlush - 1) flush();
        }
        if (nf & (kFlush - 1)) flush();                    // a short last stage that ended between two flushes
    }

    // S > 1: a partial tile, row = position in tile ti, column = position in tile tj;
    // S = 1: the pairs i < j < P straight into res[b][kq] (of a diagonal tile's skipped quarter every pair has i >= j)
    const int64_t bk = (int64_t)b * K + kq;
    double *out = S > 1 ? part + ((bk * S + s) * NP + p) * (int64_t)(kM * kNoeLagPart) : res + bk * npairs * kM;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int r = ty + 16 * a, q = tx + 16 * c;
            const int64_t i = (int64_t)ti * kTile + r, j = (int64_t)tj * kTile + q;
            if (S == 1 && (i >= j || j >= P)) continue;
            const int64_t n = S > 1 ? (int64_t)(r * kTile + q) : i * (2 * (int64_t)P - i - 1) / 2 + (j - i - 1);
#pragma unroll
            for (int m = 0; m < kM; ++m)
                out[S > 1 ? Term::part_offset(m, n) : n * kM + m] = sizeof(Real) == sizeof(double) ? (double)acc[a][c][m] : tot[a][c][m];
        }
}

// part_place is the inverse of part_offset over a whole partial tile: checked when a term is compiled
template <typename Term>
constexpr bool noe_part_layout_ok()
{
    for (int e = 0; e < Term::kSums * kNoeLagPart; ++e) {
        int m = -1, n = -1;
        Term::part_place(e, m, n);
        if (m < 0 || m >= Term::kSums || n < 0 || n >= kNoeLagPart || Term::part_offset(m, n) != e) return false;
    }
    return true;
}

// one value of a partial tile per thread (Term::part_place: which sum of which pair), Term::kSums kNoeLagPart / 256 workgroups per
// (block, lag, tile pair) in one dimension: every read of a wave is contiguous whatever the layout of the tile
template <typename Term>
__global__ __launch_bounds__(256) void k_noe_finish(const double *__restrict__ part, int P, int nT, int NP, int S, int64_t npairs,
                                                    double *__restrict__ res)
{
    constexpr int kM = Term::kSums, kPart = kM * kNoeLagPart, kGroups = kPart / 256;
    static_assert(noe_part_layout_ok<Term>(), "Term::part_place must invert Term::part_offset");
    const int64_t w = blockIdx.x / kGroups;
    const int p = (int)(w % NP);
    const int64_t bk = w / NP;
    int ti, tj;
    noe_tile_pair(p, nT, ti, tj);
    const int e = (blockIdx.x % kGroups) * 256 + threadIdx.x;
    int m, n;
    Term::part_place(e, m, n);
    const int r = n / kTile, c = n - r * kTile;
    const int64_t i = (int64_t)ti * kTile + r, j = (int64_t)tj * kTile + c;
    if (i >= P || j >= P || i >= j) return;
    const double *src = part + (bk * S * NP + p) * (int64_t)kPart + e;
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += src[(int64_t)s * NP * kPart];
    res[(bk * npairs + i * (2 * (int64_t)P - i - 1) / 2 + (j - i - 1)) * kM + m] = sum;
}
