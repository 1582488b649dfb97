// sr_noe_lagged.hip -- the all-pairs dipolar map at a few chosen lags: per frame block b = frames [s, s + n), per lag k and per pair
// i < j of P selected atoms
//
//     G_b(k)_ij = sum_{t = s}^{s + n - k - 1} [1.5 (d'(t) . d'(t + k))^2 / (r(t)^2 r(t + k)^2) - 0.5] r(t)^-3 r(t + k)^-3
//
// d = x_j - x_i of the raw float32 coordinates, r = |d|, d'(t) = R(q_t) d(t): each frame with its own quaternion, so the rotation does
// not cancel as it does in r.  G_b(0) is the map's r^-6 sum; C_dd(k) = [sum_b G_b(k) / sum_b (n_b - k)] / <r^-6> and the per-pair
// internal correlation time from it are host work (spinrelax_amd/noe.py).  The third loop of the domain that is quadratic in the
// number of spins, non-linear per pair, frame and lag like k_noe_pairs (sr_noe.hip), whose conventions and layout it keeps.
//
// Arithmetic.
//   mode 0 (Real = float), explicit operations, no contraction; d, r, ri at frame t and e, s, si at frame t + k:
//       d_a  = x_ja - x_ia,  e_a likewise                1 rounding each
//       r2   = fma(dz, dz, fma(dy, dy, dx * dx)), s2     3 roundings
//       ri   = v_rsq_f32(r2), si = v_rsq_f32(s2)         1 ulp
//       d'_a = fma(Ra0, dx, fma(Ra1, dy, Ra2 * dz)), e'_a with the matrix of frame t + k;  R = float32(R(q) in float64)
//       c    = fma(d'z, e'z, fma(d'y, e'y, d'x * e'x))
//       g    = ri * si;  x = c * g;  g3 = (g * g) * g
//       p    = fma(1.5 * x, x, -0.5);  term = p * g3
//     terms added in float32 partial sums of at most kFlush = 8 origins, which are then added to float64 registers.
//   mode 1 (Real = double): the same sequence in float64 with 1 / sqrt, accumulated in float64 directly.
//
// k_noe_lagged: one workgroup of 256 threads per (block, lag, frame split s < S, tile pair ti <= tj), tiles and threads as in
//   k_noe_pairs (32 x 32 atoms, 2 x 2 pairs per thread).  LDS holds two windows of kFB = 16 frames of the 64 atoms as float4, the
//   origins t and the frames t + k, with the 2 x 16 rotation matrices; 192 threads gather one (atom, component) of both windows,
//   32 more one quaternion each; the next stage is fetched into registers during the arithmetic.  A frame split owns a range of
//   ORIGINS (noe_lag_origins): its second window reads up to k frames past that range, never past the block's end.  The diagonal
//   tile's lower quarter is skipped; pairs with i >= j and atoms past P are computed on zeros and never written.
// k_noe_lagged_finish: adds the S partial tiles of a (block, lag, tile pair) in the order s = 0 .. S-1 into G[b][k][pair]; with S = 1
//   k_noe_lagged writes G itself.  No atomics: equal input gives bit-equal G.
// The split count is noe_ksplit(tile pairs, longest block, B) -- the map's own, WITHOUT the number of lags: what a workgroup adds, and in
//   which order, then depends on its own (block, lag, split) alone, and the value of a lag has the same bits alone and in any list.
//   (With B K in the place of B the splits, and the last bits, of a lag would move with the number of lags asked for beside it.)
#include "sr_noe_common.h"
#include <vector>

namespace {

constexpr int kTile = kNoeTile;
constexpr int kFB = 16;                     // frames per LDS stage and window
constexpr int kFlush = 8;                   // mode 0: origins per float32 partial sum
constexpr int kRows = 2 * kTile * 3;        // staged series per frame: (side, atom, component) = 192, one thread each
constexpr int kPart = kNoeLagPart;          // float64 values of one partial tile
static_assert(kRows + 2 * kFB <= 256 && kFB % kFlush == 0 && kPart % 256 == 0, "stage shape");

template <typename Real, bool ROT>
__global__ __launch_bounds__(256) void k_noe_lagged(const float *__restrict__ xyz, int64_t nAtoms, const int *__restrict__ index, int P,
                                                    const double *__restrict__ quat, const int64_t *__restrict__ blk,
                                                    const int *__restrict__ lags, int K, int nT, int NP, int S, double *__restrict__ part,
                                                    double *__restrict__ G, int64_t npairs)
{
#pragma clang fp contract(off)
    __shared__ float4 crd[2][kFB][2 * kTile];          // [0]: the origins t, [1]: the frames t + k
    __shared__ Real rot[2][kFB][12];
    const int tid = threadIdx.x;
    const int bid = blockIdx.x;
    const int p = bid % NP, s = (bid / NP) % S, kq = (bid / (NP * S)) % K, b = bid / (NP * S * K);
    int ti, tj;
    noe_tile_pair(p, nT, ti, tj);
    // origins [f0, f1) of the block that split s owns at this lag
    const int64_t start = blk[2 * b], len = blk[2 * b + 1], lag = lags[kq];
    int64_t lo, hi;
    noe_lag_origins(len, lag, S, s, lo, hi);
    const int64_t f0 = start + lo, f1 = start + hi;    // f1 + lag <= start + len

    // what this thread fetches of every stage: threads 0 .. 191 one (side, atom, component) of each frame of both windows, -1 = an
    // atom past P; threads 192 .. 223 the quaternion of one frame of one window
    int64_t src = -1;
    if (tid < kRows) {
        const int a = tid / 3, c = tid - 3 * a;
        const int g = (a < kTile ? ti * kTile + a : tj * kTile + a - kTile);
        if (g < P) src = (int64_t)index[g] * 3 + c;
    }
    const int qi = tid - kRows;                        // 0 .. 2 kFB - 1 on the quaternion threads
    const int qw = qi >= kFB ? 1 : 0, qf = qi - qw * kFB;
    float pre[2][kFB];
    double qpre[4] = {1.0, 0.0, 0.0, 0.0};
    auto fetch = [&](int64_t fs) {
        if (tid < kRows) {
#pragma unroll
            for (int f = 0; f < kFB; ++f) {
                const bool in = src >= 0 && fs + f < f1;
                pre[0][f] = in ? xyz[(fs + f) * nAtoms * 3 + src] : 0.f;
                pre[1][f] = in ? xyz[(fs + f + lag) * nAtoms * 3 + src] : 0.f;
            }
        } else if (ROT && qi < 2 * kFB && fs + qf < f1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) qpre[k] = quat[(fs + qf + (qw ? lag : 0)) * 4 + k];
        }
    };

    const int ty = tid >> 4, tx = tid & 15;
    const bool diag = ti == tj;
    Real acc[2][2];
    double tot[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) { acc[a][c] = (Real)0; tot[a][c] = 0.0; }
    auto flush = [&]() {
        if (sizeof(Real) == sizeof(double)) return;     // mode 1 accumulates in acc, which is float64
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c) { tot[a][c] += (double)acc[a][c]; acc[a][c] = (Real)0; }
    };

    if (f0 < f1) fetch(f0);
    for (int64_t fs = f0; fs < f1; fs += kFB) {
        __syncthreads();                                   // the previous stage has been read
        if (tid < kRows) {
            const int a = tid / 3, c = tid - 3 * a;
#pragma unroll
            for (int f = 0; f < kFB; ++f) {
                reinterpret_cast<float *>(&crd[0][f][a])[c] = pre[0][f];
                reinterpret_cast<float *>(&crd[1][f][a])[c] = pre[1][f];
            }
        } else if (ROT && qi < 2 * kFB) {
            const double w = qpre[0], x = qpre[1], y = qpre[2], z = qpre[3];
            Real *R = rot[qw][qf];
            R[0] = (Real)(1 - 2 * (y * y + z * z)); R[1] = (Real)(2 * (x * y - w * z));     R[2] = (Real)(2 * (x * z + w * y));
            R[4] = (Real)(2 * (x * y + w * z));     R[5] = (Real)(1 - 2 * (x * x + z * z)); R[6] = (Real)(2 * (y * z - w * x));
            R[8] = (Real)(2 * (x * z - w * y));     R[9] = (Real)(2 * (y * z + w * x));     R[10] = (Real)(1 - 2 * (x * x + y * y));
        }
        __syncthreads();
        if (fs + kFB < f1) fetch(fs + kFB);                // in flight during the arithmetic below
        const int nf = (int)(f1 - fs < kFB ? f1 - fs : (int64_t)kFB);
        for (int f = 0; f < nf; ++f) {
            float4 xi[2], xj[2], yi[2], yj[2];
            xi[0] = crd[0][f][ty]; xi[1] = crd[0][f][ty + 16];
            xj[0] = crd[0][f][kTile + tx]; xj[1] = crd[0][f][kTile + tx + 16];
            yi[0] = crd[1][f][ty]; yi[1] = crd[1][f][ty + 16];
            yj[0] = crd[1][f][kTile + tx]; yj[1] = crd[1][f][kTile + tx + 16];
            Real R[12], Q[12];
            if (ROT) {
#pragma unroll
                for (int k = 0; k < 12; ++k) { R[k] = rot[0][f][k]; Q[k] = rot[1][f][k]; }
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    if (diag && a == 1 && c == 0) continue;
                    const Real dx = (Real)xj[c].x - (Real)xi[a].x, dy = (Real)xj[c].y - (Real)xi[a].y, dz = (Real)xj[c].z - (Real)xi[a].z;
                    const Real ex = (Real)yj[c].x - (Real)yi[a].x, ey = (Real)yj[c].y - (Real)yi[a].y, ez = (Real)yj[c].z - (Real)yi[a].z;
                    const Real r2 = noe_fma(dz, dz, noe_fma(dy, dy, dx * dx));
                    const Real s2 = noe_fma(ez, ez, noe_fma(ey, ey, ex * ex));
                    const Real ri = noe_rsqrt(r2), si = noe_rsqrt(s2);
                    Real px = dx, py = dy, pz = dz, qx = ex, qy = ey, qz = ez;
                    if (ROT) {
                        px = noe_fma(R[0], dx, noe_fma(R[1], dy, R[2] * dz));
                        py = noe_fma(R[4], dx, noe_fma(R[5], dy, R[6] * dz));
                        pz = noe_fma(R[8], dx, noe_fma(R[9], dy, R[10] * dz));
                        qx = noe_fma(Q[0], ex, noe_fma(Q[1], ey, Q[2] * ez));
                        qy = noe_fma(Q[4], ex, noe_fma(Q[5], ey, Q[6] * ez));
                        qz = noe_fma(Q[8], ex, noe_fma(Q[9], ey, Q[10] * ez));
                    }
                    const Real cc = noe_fma(pz, qz, noe_fma(py, qy, px * qx));
                    const Real g = ri * si;
                    const Real x = cc * g;
                    const Real g3 = (g * g) * g;
                    const Real pp = noe_fma((Real)1.5 * x, x, (Real)-0.5);
                    acc[a][c] += pp * g3;
                }
            if ((f & (kFlush - 1)) == kFlush - 1) flush();
        }
        if (nf & (kFlush - 1)) flush();                    // a short last stage that ended between two flushes
    }

    // S > 1: a partial tile, (row, column), row = position in tile ti, column = position in tile tj;
    // S = 1: the pairs i < j < P straight into G[b][kq] (of a diagonal tile's skipped quarter every pair has i >= j)
    const int64_t bk = (int64_t)b * K + kq;
    double *out = S > 1 ? part + ((bk * S + s) * NP + p) * kPart : G + bk * npairs;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int r = ty + 16 * a, q = tx + 16 * c;
            const int64_t i = (int64_t)ti * kTile + r, j = (int64_t)tj * kTile + q;
            if (S == 1 && (i >= j || j >= P)) continue;
            out[S > 1 ? (int64_t)(r * kTile + q) : i * (2 * (int64_t)P - i - 1) / 2 + (j - i - 1)] =
                sizeof(Real) == sizeof(double) ? (double)acc[a][c] : tot[a][c];
        }
}

// one value of a tile per thread, kPart / 256 = 4 workgroups per (block, lag, tile pair): blockIdx.x = ((b K + kq) NP + p) 4 + quarter
__global__ __launch_bounds__(256) void k_noe_lagged_finish(const double *__restrict__ part, int P, int nT, int NP, int S, int64_t npairs,
                                                           double *__restrict__ G)
{
    const int64_t w = blockIdx.x >> 2;
    const int p = (int)(w % NP);
    const int64_t bk = w / NP;
    int ti, tj;
    noe_tile_pair(p, nT, ti, tj);
    const int e = (blockIdx.x & 3) * 256 + threadIdx.x;
    const int r = e / kTile, c = e - r * kTile;
    const int64_t i = (int64_t)ti * kTile + r, j = (int64_t)tj * kTile + c;
    if (i >= P || j >= P || i >= j) return;
    const double *src = part + (bk * S * NP + p) * kPart + e;
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += src[(int64_t)s * NP * kPart];
    G[bk * npairs + i * (2 * (int64_t)P - i - 1) / 2 + (j - i - 1)] = sum;
}

// everything that is refused, before anything is queued: the map's own refusals, then the lags, the memory and the grid
int noe_lagged_check(sr_ctx *ctx, const char *who, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const int64_t *bs,
                     const int64_t *bl, int B, const int32_t *lags, int K, int mode, NoeShape &sh)
{
    if (int rc = noe_check(ctx, who, nFrames, nAtoms, index, P, bs, bl, B, mode, sh)) return rc;
    int64_t shortest = bl[0];
    for (int b = 1; b < B; ++b)
        if (bl[b] < shortest) shortest = bl[b];
    char msg[160];
    if (int rc = noe_lag_check(lags, K, shortest, msg, sizeof msg)) {
        sr_set_error("%s: %s", who, msg);
        return rc;
    }
    unsigned __int128 out_bytes, part_bytes;
    noe_lagged_bytes(B, K, sh.npairs, sh.S, sh.NP, out_bytes, part_bytes);
    const unsigned __int128 have = ctx->prop.totalGlobalMem;
    SR_REQUIRE(out_bytes <= have && part_bytes <= have && out_bytes + part_bytes <= have, -3,
               "%s: %d blocks x %d lags x %lld pairs x 8 bytes = %.1f GiB of G (and %.1f GiB of partial tiles) do not fit the device's %.1f GiB", who,
               B, K, (long long)sh.npairs, (double)out_bytes / 1073741824.0, (double)part_bytes / 1073741824.0, (double)have / 1073741824.0);
    SR_REQUIRE(noe_lagged_grid_ok(B, K, sh.S, sh.NP), -3, "%s: %lld tile pairs x %d splits x %d lags x %d blocks are too many for one call", who,
               (long long)sh.NP, sh.S, K, B);
    return 0;
}

}  // namespace

extern "C" {

int sr_noe_lagged_splits(int64_t P, int64_t longest_block, int B)
{
    if (P < 2 || longest_block < 1 || B < 1) return 0;
    const int64_t nT = (P + kTile - 1) / kTile;
    return noe_ksplit(nT * (nT + 1) / 2, longest_block, B);
}

int sr_noe_lagged_check(sr_ctx *ctx, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const int64_t *block_start,
                        const int64_t *block_len, int B, const int32_t *lags, int K, int mode)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(index && block_start && block_len && (lags || K < 1), -2, "sr_noe_lagged_check: null pointer");
    NoeShape sh;
    return noe_lagged_check(ctx, "sr_noe_lagged_check", nFrames, nAtoms, index, P, block_start, block_len, B, lags, K, mode, sh);
}

int sr_noe_lagged_f32_dev(sr_ctx *ctx, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index_host, int64_t P,
                          const double *quat, const int64_t *block_start_host, const int64_t *block_len_host, int B,
                          const int32_t *lags_host, int K, int mode, double *G)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(xyz && index_host && block_start_host && block_len_host && (lags_host || K < 1) && G, -2, "sr_noe_lagged_f32_dev: null pointer");
    NoeShape sh;
    if (int rc = noe_lagged_check(ctx, "sr_noe_lagged_f32_dev", nFrames, nAtoms, index_host, P, block_start_host, block_len_host, B, lags_host, K,
                                  mode, sh))
        return rc;
    // ---- the block table, (start, length) pairs, then the atom indices and the lags; the partial tiles ----
    const size_t tab_bytes = (size_t)B * 2 * sizeof(int64_t);
    char *misc = (char *)sr_workspace(ctx, SR_WS_MISC, tab_bytes + ((size_t)P + (size_t)K) * sizeof(int));
    double *part = sh.S > 1 ? (double *)sr_workspace(ctx, SR_WS_NOE, (size_t)B * K * sh.S * sh.NP * kPart * sizeof(double)) : nullptr;
    if (!misc || (sh.S > 1 && !part)) return -5;
    int64_t *blk_dev = (int64_t *)misc;
    int *idx_dev = (int *)(misc + tab_bytes);
    int *lag_dev = idx_dev + P;
    std::vector<int64_t> table((size_t)B * 2);
    for (int b = 0; b < B; ++b) { table[2 * b] = block_start_host[b]; table[2 * b + 1] = block_len_host[b]; }
    SR_HIP(hipMemcpyAsync(blk_dev, table.data(), tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    SR_HIP(hipMemcpyAsync(idx_dev, index_host, (size_t)P * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    SR_HIP(hipMemcpyAsync(lag_dev, lags_host, (size_t)K * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    SR_HIP(hipStreamSynchronize(ctx->stream));          // small tables: the caller's arrays are free again when this returns
    // ---- launch ----
    const dim3 grid((unsigned)((int64_t)B * K * sh.S * sh.NP)), block(256);
    int rc;
#define NOE_LAUNCH(Real, ROT)                                                                                                        \
    sr_launch(ctx, k_noe_lagged<Real, ROT>, grid, block, 0, xyz, nAtoms, (const int *)idx_dev, (int)P, quat, (const int64_t *)blk_dev, \
              (const int *)lag_dev, K, (int)sh.nT, (int)sh.NP, sh.S, part, G, sh.npairs)
    if (mode == 0) rc = quat ? NOE_LAUNCH(float, true) : NOE_LAUNCH(float, false);
    else rc = quat ? NOE_LAUNCH(double, true) : NOE_LAUNCH(double, false);
#undef NOE_LAUNCH
    if (rc || sh.S == 1) return rc;
    return sr_launch(ctx, k_noe_lagged_finish, dim3((unsigned)((int64_t)B * K * sh.NP * (kPart / 256))), dim3(256), 0, (const double *)part, (int)P,
                     (int)sh.nT, (int)sh.NP, sh.S, sh.npairs, G);
}

int sr_noe_lagged_f32(sr_ctx *ctx, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const double *quat,
                      const int64_t *block_start, const int64_t *block_len, int B, const int32_t *lags, int K, int mode, double *G)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(xyz && index && block_start && block_len && (lags || K < 1) && G, -2, "sr_noe_lagged_f32: null pointer");
    NoeShape sh;
    if (int rc = noe_lagged_check(ctx, "sr_noe_lagged_f32", nFrames, nAtoms, index, P, block_start, block_len, B, lags, K, mode, sh)) return rc;
    const size_t nin = (size_t)nFrames * nAtoms * 3, nq = (size_t)nFrames * 4, nout = (size_t)B * K * sh.npairs;
    sr_stage st(ctx);
    const float *xyz_d = st.open(SR_WS_VECS, nin * sizeof(float)).put(xyz, nin);
    const double *q_d = quat ? st.open(SR_WS_IN0, nq * sizeof(double)).put(quat, nq) : nullptr;
    double *G_d = st.take<double>(SR_WS_OUT0, nout);
    if (st.rc) return st.rc;
    if (int rc = sr_noe_lagged_f32_dev(ctx, xyz_d, nFrames, nAtoms, index, P, q_d, block_start, block_len, B, lags, K, mode, G_d)) return rc;
    st.fetch(G, G_d, nout);
    return st.finish();
}

}  // extern "C"
