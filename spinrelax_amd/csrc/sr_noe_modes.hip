// sr_noe_modes.hip -- the lagged all-pairs dipolar map (sr_noe_lagged.hip) split into the five tumbling modes of an anisotropic
// rotational diffusion tensor: per frame block b = frames [s, s + n), per lag k and per pair i < j of P selected atoms the six sums
//
//     H0 = sum w qz(u) qz(v)        H1 = sum w dl(u) dl(v)        H2 = sum w [qz(u) dl(v) + dl(u) qz(v)] / 2
//     H3 = sum w uy uz vy vz        H4 = sum w ux uz vx vz        H5 = sum w ux uy vx vy
//
// over the origins t = s .. s + n - k - 1, with d = x_j - x_i of the raw float32 coordinates, r = |d|, d"(t) = F R(q_t) d(t) (each
// frame with its own quaternion, F = R(q_F) the constant rotation into the tensor's principal-axis frame), u = d"(t) / r(t),
// v = d"(t + k) / r(t + k), w = r(t)^-3 r(t + k)^-3, qz(u) = uz^2 - 1/3 and dl(u) = ux^2 - uy^2.  The sums do not depend on the tensor;
// the amplitudes of its five modes are linear in them (spinrelax_amd/noe.py: mode_amplitudes).  With Q = u u^T - 1/3:
// P2(u . v) = 1.5 Q : Q' = 2.25 qz qz' + 0.75 dl dl' + 3 (uy uz vy vz + ux uz vx vz + ux uy vx vy), so that
// 2.25 H0 + 0.75 H1 + 3 (H3 + H4 + H5) = G of k_noe_lagged, whatever F.  Conventions and layout are k_noe_lagged's.
//
// Arithmetic.
//   mode 0 (Real = float), explicit operations, no contraction; d, r, ri at frame t and e, s, si at frame t + k:
//       d_a  = x_ja - x_ia,  e_a likewise                1 rounding each
//       r2   = fma(dz, dz, fma(dy, dy, dx * dx)), s2     3 roundings
//       ri   = v_rsq_f32(r2), si = v_rsq_f32(s2)         1 ulp
//       d'_a = fma(Ma0, dx, fma(Ma1, dy, Ma2 * dz)), e'_a with the matrix of frame t + k;  M = float32(F R(q) in float64)
//       u_a  = d'_a * ri,  v_a = e'_a * si
//       a0   = fma(uz, uz, -1/3),  a1 = fma(ux, ux, -(uy * uy));  b0, b1 of v likewise
//       g    = ri * si;  g3 = (g * g) * g
//       t0 = (a0 * b0) * g3;  t1 = (a1 * b1) * g3;  t2 = (0.5 * fma(a0, b1, a1 * b0)) * g3
//       t3 = ((uy * uz) * (vy * vz)) * g3;  t4 = ((ux * uz) * (vx * vz)) * g3;  t5 = ((ux * uy) * (vx * vy)) * g3
//     terms added in float32 partial sums of at most kFlush = 8 origins, which are then added to float64 registers.
//   mode 1 (Real = double): the same sequence in float64 with 1 / sqrt, accumulated in float64 directly.
//
// k_noe_modes: one workgroup of 256 threads per (block, lag, frame split s < S, tile pair ti <= tj): the tiles (32 x 32 atoms, 2 x 2
//   pairs per thread), the two LDS windows of kFB = 16 frames, the gather threads, the prefetch and the origin ranges
//   (noe_lag_origins) of k_noe_lagged.  The 32 quaternion threads compose F into their frame's matrix, F R(q_t) in float64, rounded
//   to Real once; without quaternions R(q_t) = 1 and the matrix is F; without either the no-rotation instantiation runs.
// k_noe_modes_finish: adds the S partial tiles of a (block, lag, tile pair) in the order s = 0 .. S-1 into H[b][k][pair][0 .. 5]; with
//   S = 1 k_noe_modes writes H itself.  No atomics: equal input gives bit-equal H.
// The split count is noe_ksplit(tile pairs, longest block, B), the map's own, without the number of lags: the value of a lag has the
//   same bits alone and in any list.
#include "sr_noe_common.h"
#include <vector>

namespace {

constexpr int kTile = kNoeTile;
constexpr int kFB = 16;                     // frames per LDS stage and window
constexpr int kFlush = 8;                   // mode 0: origins per float32 partial sum
constexpr int kRows = 2 * kTile * 3;        // staged series per frame: (side, atom, component) = 192, one thread each
constexpr int kPart = kNoeLagPart;          // float64 values of one sum of one partial tile
constexpr int kM = kNoeModeSums;            // sums per pair
static_assert(kRows + 2 * kFB <= 256 && kFB % kFlush == 0 && kPart % 256 == 0, "stage shape");

struct FrameMat {
    double m[9];                            // F, row-major
};

template <typename Real, bool ROT>
__global__ __launch_bounds__(256) void k_noe_modes(const float *__restrict__ xyz, int64_t nAtoms, const int *__restrict__ index, int P,
                                                   const double *__restrict__ quat, FrameMat F, const int64_t *__restrict__ blk,
                                                   const int *__restrict__ lags, int K, int nT, int NP, int S, double *__restrict__ part,
                                                   double *__restrict__ H, int64_t npairs)
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
    double qpre[4] = {1.0, 0.0, 0.0, 0.0};             // without quaternions it stays the identity: the matrix is F
    auto fetch = [&](int64_t fs) {
        if (tid < kRows) {
#pragma unroll
            for (int f = 0; f < kFB; ++f) {
                const bool in = src >= 0 && fs + f < f1;
                pre[0][f] = in ? xyz[(fs + f) * nAtoms * 3 + src] : 0.f;
                pre[1][f] = in ? xyz[(fs + f + lag) * nAtoms * 3 + src] : 0.f;
            }
        } else if (ROT && quat && qi < 2 * kFB && fs + qf < f1) {
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
                reinterpret_cast<float *>(&crd[1][f][a])[c] = pre[1][f];
            }
        } else if (ROT && qi < 2 * kFB) {
            const double w = qpre[0], x = qpre[1], y = qpre[2], z = qpre[3];
            double A[9];
            A[0] = 1 - 2 * (y * y + z * z); A[1] = 2 * (x * y - w * z);     A[2] = 2 * (x * z + w * y);
            A[3] = 2 * (x * y + w * z);     A[4] = 1 - 2 * (x * x + z * z); A[5] = 2 * (y * z - w * x);
            A[6] = 2 * (x * z - w * y);     A[7] = 2 * (y * z + w * x);     A[8] = 1 - 2 * (x * x + y * y);
            Real *R = rot[qw][qf];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)                // F R(q_t) in float64, rounded to Real once
                    R[4 * r + c] = (Real)__builtin_fma(F.m[3 * r + 2], A[6 + c], __builtin_fma(F.m[3 * r + 1], A[3 + c], F.m[3 * r] * A[c]));
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
                    const Real ux = px * ri, uy = py * ri, uz = pz * ri;
                    const Real vx = qx * si, vy = qy * si, vz = qz * si;
                    const Real third = (Real)(-1.0 / 3.0);
                    const Real a0 = noe_fma(uz, uz, third), a1 = noe_fma(ux, ux, -(uy * uy));
                    const Real b0 = noe_fma(vz, vz, third), b1 = noe_fma(vx, vx, -(vy * vy));
                    const Real g = ri * si;
                    const Real g3 = (g * g) * g;
                    acc[a][c][0] += (a0 * b0) * g3;
                    acc[a][c][1] += (a1 * b1) * g3;
                    acc[a][c][2] += ((Real)0.5 * noe_fma(a0, b1, a1 * b0)) * g3;
                    acc[a][c][3] += ((uy * uz) * (vy * vz)) * g3;
                    acc[a][c][4] += ((ux * uz) * (vx * vz)) * g3;
                    acc[a][c][5] += ((ux * uy) * (vx * vy)) * g3;
                }
            if ((f & (kFlush - 1)) == kFlush - 1) flush();
        }
        if (nf & (kFlush - 1)) flush();                    // a short last stage that ended between two flushes
    }

    // S > 1: a partial tile, [sum][row][column], row = position in tile ti, column = position in tile tj;
    // S = 1: the pairs i < j < P straight into H[b][kq] (of a diagonal tile's skipped quarter every pair has i >= j)
    const int64_t bk = (int64_t)b * K + kq;
    double *out = S > 1 ? part + ((bk * S + s) * NP + p) * (int64_t)(kM * kPart) : H + bk * npairs * kM;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int r = ty + 16 * a, q = tx + 16 * c;
            const int64_t i = (int64_t)ti * kTile + r, j = (int64_t)tj * kTile + q;
            if (S == 1 && (i >= j || j >= P)) continue;
            const int64_t pair = i * (2 * (int64_t)P - i - 1) / 2 + (j - i - 1);
#pragma unroll
            for (int m = 0; m < kM; ++m)
                out[S > 1 ? (int64_t)(m * kPart + r * kTile + q) : pair * kM + m] =
                    sizeof(Real) == sizeof(double) ? (double)acc[a][c][m] : tot[a][c][m];
        }
}

// the six sums of one pair of a tile per thread, kPart / 256 = 4 workgroups per (block, lag, tile pair):
// blockIdx.x = ((b K + kq) NP + p) 4 + quarter
__global__ __launch_bounds__(256) void k_noe_modes_finish(const double *__restrict__ part, int P, int nT, int NP, int S, int64_t npairs,
                                                          double *__restrict__ H)
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
    const double *src = part + (bk * S * NP + p) * (int64_t)(kM * kPart) + e;
    double *dst = H + (bk * npairs + i * (2 * (int64_t)P - i - 1) / 2 + (j - i - 1)) * kM;
#pragma unroll
    for (int m = 0; m < kM; ++m) {
        double sum = 0.0;
        for (int s = 0; s < S; ++s) sum += src[(int64_t)s * NP * (kM * kPart) + m * kPart];
        dst[m] = sum;
    }
}

// everything that is refused, before anything is queued: the map's own refusals, then the lags, the frame quaternion, the memory and
// the grid; fills sh and F
int noe_modes_check(sr_ctx *ctx, const char *who, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const int64_t *bs,
                    const int64_t *bl, int B, const int32_t *lags, int K, const double *frame_quat, int mode, NoeShape &sh, FrameMat &F)
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
    if (int rc = noe_frame_matrix(frame_quat, F.m, msg, sizeof msg)) {
        sr_set_error("%s: %s", who, msg);
        return rc;
    }
    unsigned __int128 out_bytes, part_bytes;
    noe_modes_bytes(B, K, sh.npairs, sh.S, sh.NP, out_bytes, part_bytes);
    const unsigned __int128 have = ctx->prop.totalGlobalMem;
    SR_REQUIRE(out_bytes <= have && part_bytes <= have && out_bytes + part_bytes <= have, -3,
               "%s: %d blocks x %d lags x %lld pairs x 6 x 8 bytes = %.1f GiB of H (and %.1f GiB of partial tiles) do not fit the device's %.1f GiB",
               who, B, K, (long long)sh.npairs, (double)out_bytes / 1073741824.0, (double)part_bytes / 1073741824.0, (double)have / 1073741824.0);
    SR_REQUIRE(noe_modes_grid_ok(B, K, sh.S, sh.NP), -3, "%s: %lld tile pairs x %d splits x %d lags x %d blocks are too many for one call", who,
               (long long)sh.NP, sh.S, K, B);
    return 0;
}

}  // namespace

extern "C" {

int sr_noe_modes_check(sr_ctx *ctx, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const int64_t *block_start,
                       const int64_t *block_len, int B, const int32_t *lags, int K, const double *frame_quat, int mode)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(index && block_start && block_len && (lags || K < 1), -2, "sr_noe_modes_check: null pointer");
    NoeShape sh;
    FrameMat F;
    return noe_modes_check(ctx, "sr_noe_modes_check", nFrames, nAtoms, index, P, block_start, block_len, B, lags, K, frame_quat, mode, sh, F);
}

int sr_noe_modes_f32_dev(sr_ctx *ctx, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index_host, int64_t P,
                         const double *quat, const double *frame_quat_host, const int64_t *block_start_host, const int64_t *block_len_host,
                         int B, const int32_t *lags_host, int K, int mode, double *H)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(xyz && index_host && block_start_host && block_len_host && (lags_host || K < 1) && H, -2, "sr_noe_modes_f32_dev: null pointer");
    NoeShape sh;
    FrameMat F;
    if (int rc = noe_modes_check(ctx, "sr_noe_modes_f32_dev", nFrames, nAtoms, index_host, P, block_start_host, block_len_host, B, lags_host, K,
                                 frame_quat_host, mode, sh, F))
        return rc;
    // ---- the block table, (start, length) pairs, then the atom indices and the lags; the partial tiles ----
    const size_t tab_bytes = (size_t)B * 2 * sizeof(int64_t);
    char *misc = (char *)sr_workspace(ctx, SR_WS_MISC, tab_bytes + ((size_t)P + (size_t)K) * sizeof(int));
    double *part = sh.S > 1 ? (double *)sr_workspace(ctx, SR_WS_NOE, (size_t)B * K * sh.S * sh.NP * kM * kPart * sizeof(double)) : nullptr;
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
    const bool rotate = quat || frame_quat_host;
    int rc;
#define NOE_LAUNCH(Real, ROT)                                                                                                          \
    sr_launch(ctx, k_noe_modes<Real, ROT>, grid, block, 0, xyz, nAtoms, (const int *)idx_dev, (int)P, quat, F, (const int64_t *)blk_dev, \
              (const int *)lag_dev, K, (int)sh.nT, (int)sh.NP, sh.S, part, H, sh.npairs)
    if (mode == 0) rc = rotate ? NOE_LAUNCH(float, true) : NOE_LAUNCH(float, false);
    else rc = rotate ? NOE_LAUNCH(double, true) : NOE_LAUNCH(double, false);
#undef NOE_LAUNCH
    if (rc || sh.S == 1) return rc;
    return sr_launch(ctx, k_noe_modes_finish, dim3((unsigned)((int64_t)B * K * sh.NP * (kPart / 256))), dim3(256), 0, (const double *)part, (int)P,
                     (int)sh.nT, (int)sh.NP, sh.S, sh.npairs, H);
}

int sr_noe_modes_f32(sr_ctx *ctx, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const double *quat,
                     const double *frame_quat, const int64_t *block_start, const int64_t *block_len, int B, const int32_t *lags, int K, int mode,
                     double *H)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(xyz && index && block_start && block_len && (lags || K < 1) && H, -2, "sr_noe_modes_f32: null pointer");
    NoeShape sh;
    FrameMat F;
    if (int rc = noe_modes_check(ctx, "sr_noe_modes_f32", nFrames, nAtoms, index, P, block_start, block_len, B, lags, K, frame_quat, mode, sh, F))
        return rc;
    const size_t nin = (size_t)nFrames * nAtoms * 3, nq = (size_t)nFrames * 4, nout = (size_t)B * K * sh.npairs * kM;
    sr_stage st(ctx);
    const float *xyz_d = st.open(SR_WS_VECS, nin * sizeof(float)).put(xyz, nin);
    const double *q_d = quat ? st.open(SR_WS_IN0, nq * sizeof(double)).put(quat, nq) : nullptr;
    double *H_d = st.take<double>(SR_WS_OUT0, nout);
    if (st.rc) return st.rc;
    if (int rc = sr_noe_modes_f32_dev(ctx, xyz_d, nFrames, nAtoms, index, P, q_d, frame_quat, block_start, block_len, B, lags, K, mode, H_d)) return rc;
    st.fetch(H, H_d, nout);
    return st.finish();
}

}  // extern "C"
