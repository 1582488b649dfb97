// sr_ired.hip -- iRED: the equal-time P2 cross-correlation matrix of the bond vectors, per window of frames
//
//     M[w][i][j] = (1 / F_w) sum_t ( 1.5 (u_i(t) . u_j(t))^2 - 0.5 )          (Prompers & Brueschweiler, JACS 2002;
//                                                                              windows: Gu, Li & Brueschweiler, JCTC 2014)
// The reference names the analysis (calculate_S2_by_iRED / calculate_S2_by_wiRED, calculate-S2.py:158-191) and stops after the
// window length; this is built to the publications.  It is the one loop of the domain that is quadratic in the number of vectors.
//
// Formulation.  (u_i.u_j)^2 = sum_{a<=b} w_ab (u_ia u_ib)(u_ja u_jb), w = 1 for xx, yy, zz and 2 for xy, xz, yz: the sum over a
// window's frames is a symmetric rank-k update Q = A B with K = 6 F_w, A[i][(t, ab)] = u_ia(t) u_ib(t) and B = w A^T.  A product of two
// float32 values is exact in float64 and so is its double, so the operands carry no rounding at all; the only rounding is the
// float64 accumulation of the matrix pipe.
//
// k_ired_matrix: one workgroup (4 waves) per (window, tile pair with tile row <= tile column, frame split).  A tile is 64 x 64, a wave
//   owns a 32 x 32 quarter as 2 x 2 accumulators of v_mfma_f64_16x16x4_f64.  One MFMA covers 4 frames of one component pair:
//   lane l gives A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], so a lane reads x, y, z of ONE vector at ONE frame from
//   LDS (float32) and forms its six operands in registers; the six-component array never exists in memory.
//   LDS holds kT = 20 frames of the 64 row and the 64 column vectors as [side][vector][component][frame]: a vector is 60 floats
//   on, and 16 vectors x 4 frames of a read fall on 64 different banks (60 r + k mod 64); the next stage is fetched into
//   registers while the current one is multiplied.  Vectors past nV and frames past the split's range are staged as zeros, which
//   add exactly 0.
//   The accumulator map of the f64 instruction is col = lane & 15, row = (lane >> 4) + 4 reg (NOT the f32 one).
// k_ired_finish: adds the S partial tiles of a (window, tile pair) in the order s = 0 .. S-1, applies 1.5 / F_w and -0.5 and writes
//   M[i][j] and M[j][i] from the same value (of a diagonal tile only i <= j is taken): M is exactly symmetric.
// No atomics anywhere: equal input and equal S give bit-equal M.
#include "sr_internal.h"
#include <vector>

namespace {

constexpr int kTile = 64;                   // vectors per tile side
constexpr int kT = 20;                      // frames per LDS stage: a multiple of 4 (one MFMA k-step), kT = 4 mod 8 (banks, see above)
constexpr int kRows = 2 * kTile * 3;        // staged series: (side, vector, component)
constexpr int kStage = kRows * kT;          // floats per stage
constexpr int kPerThread = kStage / 256;    // 30
static_assert(kStage % 256 == 0 && kT % 4 == 0 && kT % 8 == 4, "stage shape");

typedef double d4 __attribute__((ext_vector_type(4)));

// tile pair p = 0 .. T (T + 1) / 2 - 1, row-major over ti <= tj
__device__ __forceinline__ void ired_pair(int p, int T, int &ti, int &tj)
{
    ti = 0;
    while (p >= T - ti) { p -= T - ti; ++ti; }
    tj = ti + p;
}

// frames [f0, f1) of window (start, len) that split s of S owns: runs of ceil(len / S) rounded up to whole k-steps
__device__ __forceinline__ void ired_range(int64_t start, int64_t len, int s, int S, int64_t &f0, int64_t &f1)
{
    const int64_t per = ((len + S - 1) / S + 3) / 4 * 4;
    const int64_t a = (int64_t)s * per, b = a + per;
    f0 = start + (a < len ? a : len);
    f1 = start + (b < len ? b : len);
}

__global__ __launch_bounds__(256) void k_ired_matrix(const float *__restrict__ soa, int64_t Npad, int nV, const int64_t *__restrict__ win,
                                                     int W, int T, int P, int S, double *__restrict__ part)
{
    __shared__ float lds[kStage];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bid = blockIdx.x;
    const int p = bid % P, s = (bid / P) % S, w = bid / (P * S);
    int ti, tj;
    ired_pair(p, T, ti, tj);
    int64_t f0, f1;
    ired_range(win[2 * w], win[2 * w + 1], s, S, f0, f1);

    // what this thread fetches of every stage: element q of it is series row_q at frame t_q; -1 = a vector past nV
    int64_t src[kPerThread];
    int tq[kPerThread];
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
        const int idx = tid + 256 * q, row = idx / kT;
        tq[q] = idx - row * kT;
        const int side = row / (3 * kTile), vc = row - side * 3 * kTile, v = vc / 3, c = vc - 3 * v;
        const int gv = (side ? tj : ti) * kTile + v;
        src[q] = gv < nV ? ((int64_t)gv * 3 + c) * Npad : -1;
    }
    float pre[kPerThread];
    auto fetch = [&](int64_t fs) {
#pragma unroll
        for (int q = 0; q < kPerThread; ++q) {
            const int64_t f = fs + tq[q];
            pre[q] = (src[q] >= 0 && f < f1) ? soa[src[q] + f] : 0.f;
        }
    };

    d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};

    // this lane's operand sources: vector (lane & 15) of each of the wave's two 16-row and two 16-column groups, frame lane >> 4
    const int wr = wave >> 1, wc = wave & 1, lv = lane & 15, lk = lane >> 4;
    const float *rowp[2], *colp[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        rowp[g] = lds + ((0 * kTile + wr * 32 + g * 16 + lv) * 3) * kT + lk;
        colp[g] = lds + ((1 * kTile + wc * 32 + g * 16 + lv) * 3) * kT + lk;
    }

    if (f0 < f1) fetch(f0);
    for (int64_t fs = f0; fs < f1; fs += kT) {
        __syncthreads();                                   // the previous stage has been read
#pragma unroll
        for (int q = 0; q < kPerThread; ++q) lds[tid + 256 * q] = pre[q];
        __syncthreads();
        if (fs + kT < f1) fetch(fs + kT);                  // in flight during the products below
        const int steps = (int)((f1 - fs < kT ? f1 - fs : (int64_t)kT) + 3) / 4;
        for (int k = 0; k < steps; ++k) {
            double A[2][6], B[2][6];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const double x = rowp[g][4 * k], y = rowp[g][kT + 4 * k], z = rowp[g][2 * kT + 4 * k];
                A[g][0] = x * x; A[g][1] = y * y; A[g][2] = z * z;
                A[g][3] = x * y; A[g][4] = x * z; A[g][5] = y * z;
                const double u = colp[g][4 * k], v = colp[g][kT + 4 * k], t = colp[g][2 * kT + 4 * k];
                const double u2 = u + u, v2 = v + v;          // the weight 2 of the mixed terms, on this side only
                B[g][0] = u * u; B[g][1] = v * v; B[g][2] = t * t;
                B[g][3] = u2 * v; B[g][4] = u2 * t; B[g][5] = v2 * t;
            }
#pragma unroll
            for (int c = 0; c < 6; ++c)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(A[a][c], B[b][c], acc[a][b], 0, 0, 0);
        }
    }

    // partial tile, row-major 64 x 64; f64 accumulator map: col = lane & 15, row = (lane >> 4) + 4 reg
    double *out = part + ((int64_t)(w * P + p) * S + s) * (kTile * kTile);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr * 32 + a * 16 + lk + 4 * r, col = wc * 32 + b * 16 + lv;
                out[row * kTile + col] = acc[a][b][r];
            }
}

__global__ __launch_bounds__(256) void k_ired_finish(const double *__restrict__ part, const int64_t *__restrict__ win, int nV, int T,
                                                     int P, int S, double *__restrict__ M)
{
    const int p = blockIdx.x, w = blockIdx.y;
    int ti, tj;
    ired_pair(p, T, ti, tj);
    const double scale = 1.5 / (double)win[2 * w + 1];
    const double *src = part + (int64_t)(w * P + p) * S * (kTile * kTile);
    double *Mw = M + (int64_t)w * nV * nV;
    for (int e = threadIdx.x; e < kTile * kTile; e += 256) {
        const int r = e / kTile, c = e - r * kTile;
        const int64_t i = (int64_t)ti * kTile + r, j = (int64_t)tj * kTile + c;
        if (i >= nV || j >= nV || (ti == tj && r > c)) continue;
        double sum = 0.0;
        for (int s = 0; s < S; ++s) sum += src[(int64_t)s * (kTile * kTile) + e];
        const double m = sum * scale - 0.5;
        Mw[i * nV + j] = m;
        Mw[j * nV + i] = m;
    }
}

}  // namespace

// the split rule: a function of the shape alone (never of the device or of a timing): about four workgroups per CU of a 256-CU part,
// each with at least 256 frames, at most 64 partial tiles to add
static int ired_ksplit(int64_t pairs, int64_t Fmax, int W)
{
    int64_t S = (1024 + pairs * W - 1) / (pairs * W);
    const int64_t by_frames = Fmax / 256 > 1 ? Fmax / 256 : 1;
    if (S > by_frames) S = by_frames;
    if (S > 64) S = 64;
    return (int)S;
}

extern "C" {

int sr_ired_matrix_f32_dev(sr_ctx *ctx, const float *soa, int64_t Npad, int64_t nV, const int64_t *win_start_host,
                           const int64_t *win_len_host, int W, double *M_dev)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(soa && win_start_host && win_len_host && M_dev, -2, "sr_ired_matrix_f32_dev: null pointer");
    SR_REQUIRE(nV >= 1 && W >= 1 && Npad >= 1, -3, "sr_ired_matrix_f32_dev: bad shape nV=%lld W=%d Npad=%lld", (long long)nV, W,
               (long long)Npad);
    SR_REQUIRE(nV <= 32768, -3, "sr_ired_matrix_f32_dev: nV=%lld vectors; at most 32768", (long long)nV);
    int64_t Fmax = 0;
    for (int w = 0; w < W; ++w) {
        const int64_t a = win_start_host[w], n = win_len_host[w];
        SR_REQUIRE(n >= 1, -3, "sr_ired_matrix_f32_dev: window %d has length %lld", w, (long long)n);
        SR_REQUIRE(a >= 0 && a <= Npad && n <= Npad - a, -3, "sr_ired_matrix_f32_dev: window %d = frames [%lld, %lld) is outside the %lld held",
                   w, (long long)a, (long long)(a + n), (long long)Npad);
        if (n > Fmax) Fmax = n;
    }
    const int64_t T = (nV + kTile - 1) / kTile, P = T * (T + 1) / 2;
    const int S = ctx->ired_ksplit > 0 ? ctx->ired_ksplit : ired_ksplit(P, Fmax, W);
    SR_REQUIRE(P * S * W < (int64_t)1 << 31 && W <= 65535, -3, "sr_ired_matrix_f32_dev: %lld tile pairs x %d splits x %d windows are too many for one call",
               (long long)P, S, W);
    // ---- the window table, (start, length) pairs, and the partial tiles ----
    int64_t *win_dev = (int64_t *)sr_workspace(ctx, SR_WS_MISC, (size_t)W * 2 * sizeof(int64_t));
    double *part = (double *)sr_workspace(ctx, SR_WS_IRED, (size_t)(P * S * W) * kTile * kTile * sizeof(double));
    if (!win_dev || !part) return -5;
    std::vector<int64_t> table((size_t)W * 2);
    for (int w = 0; w < W; ++w) { table[2 * w] = win_start_host[w]; table[2 * w + 1] = win_len_host[w]; }
    SR_HIP(hipMemcpyAsync(win_dev, table.data(), table.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    SR_HIP(hipStreamSynchronize(ctx->stream));          // tiny table: the caller's arrays are free again when this returns
    // ---- launch ----
    if (int rc = sr_launch(ctx, k_ired_matrix, dim3((unsigned)(P * S * W)), dim3(256), 0, soa, Npad, (int)nV, (const int64_t *)win_dev, W,
                           (int)T, (int)P, S, part))
        return rc;
    return sr_launch(ctx, k_ired_finish, dim3((unsigned)P, (unsigned)W), dim3(256), 0, (const double *)part, (const int64_t *)win_dev, (int)nV,
                     (int)T, (int)P, S, M_dev);
}

}  // extern "C"
