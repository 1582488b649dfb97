// sr_noe.hip -- all-pairs dipolar map: per frame block and per pair i < j of P selected atoms the sums over the block's frames of
//
//     r^-6     and     d'_a d'_b r^-5   (ab = xx, yy, zz, xy, xz, yz),        d = x_j - x_i,  r = |d|,  d' = R(q_t) d
//
// (Brueschweiler et al., JACS 1992; Peter, Daura & van Gunsteren, J. Biomol. NMR 2001).  <r^-6>, <r^-3> = tr T, the effective distances
// and the order parameters S2_ij = 1.5 (T:T - A3^2 / 3) / A6, S2_rad = A3^2 / A6 are host work (spinrelax_amd/noe.py).  The second loop
// of the domain that is quadratic in the number of spins; unlike the iRED matrix it is non-linear per pair and frame (a reciprocal
// square root and its powers): vector ALU work, about 30 instructions per pair and frame, nothing for the matrix pipe.
//
// Arithmetic.  d is the difference of the raw float32 coordinates, taken first and in the lab frame: r and every power of it come
// from that difference, and only the tensor sees the rotation, applied to d.  (Rotating the coordinates first would round relative to
// a coordinate of several nm what is then compared over 0.2 nm, and r^-6 multiplies that by six.)
//   mode 0 (Real = float), explicit operations, no contraction:
//       d_a  = x_ja - x_ia                               1 rounding each
//       r2   = fma(dz, dz, fma(dy, dy, dx * dx))         3 roundings
//       ri   = v_rsq_f32(r2)                             1 ulp
//       ri2  = ri * ri,  ri3 = ri2 * ri,  ri5 = ri3 * ri2,  ri6 = ri3 * ri3
//       d'_a = fma(Ra0, dx, fma(Ra1, dy, Ra2 * dz))      R = float32(R(q) in float64)
//       s_a  = d'_a * ri5;   sums: += ri6, fma(s_a, d'_b, .)
//     in float32 partial sums of at most kFlush = 8 frames, which are then added to float64 registers.
//   mode 1 (Real = double): the same sequence in float64 with 1 / sqrt, accumulated in float64 directly.
//
// k_noe_pairs: one workgroup of 256 threads per (block, frame split s < S, tile pair ti <= tj); a tile is kTile = 32 atoms, a thread
//   owns the 2 x 2 pairs (ty + 16 a, tx + 16 b), ty = tid / 16, tx = tid % 16.  LDS holds kFB = 16 frames of the 64 atoms as float4
//   (x, y, z, -): a wave reads its i-atoms as 4 broadcast addresses and its j-atoms as 16 consecutive float4 (256 contiguous bytes, each
//   read by 4 lanes).  The atoms are gathered from xyz by index while they are staged (192 threads, one (atom, component) each);
//   16 more threads fetch the frames' quaternions and store the rotation matrices (12 Reals per frame, rows padded to 4), which every
//   thread then reads as broadcasts.  The next stage is fetched into registers while the current one is worked on.
//   Of a diagonal tile the quarter a = 1, b = 0 lies wholly below the diagonal and is skipped (a uniform branch); the other pairs with
//   i >= j and the pairs of atoms past P are computed on whatever was staged (zeros: r = 0, non-finite) and never written out.
// k_noe_finish: adds the S partial tiles of a (block, tile pair) in the order s = 0 .. S-1 and writes the pairs i < j < P into
//   sums[b][i (2 P - i - 1) / 2 + j - i - 1][7].  With S = 1 (few frames, or so many tile pairs that they fill the chip alone: every
//   large map) there are no partial tiles: k_noe_pairs writes its pairs i < j < P into sums itself, and the call needs no memory
//   beside its result.
// No atomics anywhere: equal input gives bit-equal sums.
#include "sr_noe_common.h"
#include <vector>

namespace {

constexpr int kTile = kNoeTile;             // atoms per tile side (sr_noe_host.h)
constexpr int kFB = 16;                     // frames per LDS stage
constexpr int kFlush = 8;                   // mode 0: frames per float32 partial sum
constexpr int kRows = 2 * kTile * 3;        // staged series per frame: (side, atom, component) = 192, one thread each
constexpr int kPart = kTile * kTile * 7;    // float64 values of one partial tile
static_assert(kRows + kFB <= 256 && kFB % kFlush == 0 && kPart % 256 == 0, "stage shape");

template <typename Real, bool ROT>
__global__ __launch_bounds__(256) void k_noe_pairs(const float *__restrict__ xyz, int64_t nAtoms, const int *__restrict__ index, int P,
                                                   const double *__restrict__ quat, const int64_t *__restrict__ blk, int nT, int NP, int S,
                                                   double *__restrict__ part, double *__restrict__ sums, int64_t npairs)
{
#pragma clang fp contract(off)
    __shared__ float4 crd[kFB][2 * kTile];
    __shared__ Real rot[kFB][12];
    const int tid = threadIdx.x;
    const int bid = blockIdx.x;
    const int p = bid % NP, s = (bid / NP) % S, b = bid / (NP * S);
    int ti, tj;
    noe_tile_pair(p, nT, ti, tj);
    // frames [f0, f1) of the block that split s owns: runs of ceil(len / S)
    const int64_t start = blk[2 * b], len = blk[2 * b + 1];
    const int64_t per = (len + S - 1) / S;
    const int64_t lo = (int64_t)s * per, hi = lo + per;
    const int64_t f0 = start + (lo < len ? lo : len), f1 = start + (hi < len ? hi : len);

    // what this thread fetches of every stage: threads 0 .. 191 one (side, atom, component) of each frame, -1 = an atom past P;
    // threads 192 .. 207 the quaternion of one frame
    int64_t src = -1;
    if (tid < kRows) {
        const int a = tid / 3, c = tid - 3 * a;
        const int g = (a < kTile ? ti * kTile + a : tj * kTile + a - kTile);
        if (g < P) src = (int64_t)index[g] * 3 + c;
    }
    const int qf = tid - kRows;              // 0 .. kFB - 1 on the quaternion threads
    float pre[kFB];
    double qpre[4] = {1.0, 0.0, 0.0, 0.0};
    auto fetch = [&](int64_t fs) {
        if (tid < kRows) {
#pragma unroll
            for (int f = 0; f < kFB; ++f) pre[f] = (src >= 0 && fs + f < f1) ? xyz[(fs + f) * nAtoms * 3 + src] : 0.f;
        } else if (ROT && qf < kFB && fs + qf < f1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) qpre[k] = quat[(fs + qf) * 4 + k];
        }
    };

    const int ty = tid >> 4, tx = tid & 15;
    const bool diag = ti == tj;
    Real acc[2][2][7];
    double tot[2][2][7];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int k = 0; k < 7; ++k) { acc[a][c][k] = (Real)0; tot[a][c][k] = 0.0; }
    auto flush = [&]() {
        if (sizeof(Real) == sizeof(double)) return;     // mode 1 accumulates in acc, which is float64
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int k = 0; k < 7; ++k) { tot[a][c][k] += (double)acc[a][c][k]; acc[a][c][k] = (Real)0; }
    };

    if (f0 < f1) fetch(f0);
    for (int64_t fs = f0; fs < f1; fs += kFB) {
        __syncthreads();                                   // the previous stage has been read
        if (tid < kRows) {
            const int a = tid / 3, c = tid - 3 * a;
#pragma unroll
            for (int f = 0; f < kFB; ++f) reinterpret_cast<float *>(&crd[f][a])[c] = pre[f];
        } else if (ROT && qf < kFB) {
            const double w = qpre[0], x = qpre[1], y = qpre[2], z = qpre[3];
            Real *R = rot[qf];
            R[0] = (Real)(1 - 2 * (y * y + z * z)); R[1] = (Real)(2 * (x * y - w * z));     R[2] = (Real)(2 * (x * z + w * y));
            R[4] = (Real)(2 * (x * y + w * z));     R[5] = (Real)(1 - 2 * (x * x + z * z)); R[6] = (Real)(2 * (y * z - w * x));
            R[8] = (Real)(2 * (x * z - w * y));     R[9] = (Real)(2 * (y * z + w * x));     R[10] = (Real)(1 - 2 * (x * x + y * y));
        }
        __syncthreads();
        if (fs + kFB < f1) fetch(fs + kFB);                // in flight during the arithmetic below
        const int nf = (int)(f1 - fs < kFB ? f1 - fs : (int64_t)kFB);
        for (int f = 0; f < nf; ++f) {
            float4 xi[2], xj[2];
            xi[0] = crd[f][ty]; xi[1] = crd[f][ty + 16];
            xj[0] = crd[f][kTile + tx]; xj[1] = crd[f][kTile + tx + 16];
            Real R[12];
            if (ROT) {
#pragma unroll
                for (int k = 0; k < 12; ++k) R[k] = rot[f][k];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    if (diag && a == 1 && c == 0) continue;
                    const Real dx = (Real)xj[c].x - (Real)xi[a].x, dy = (Real)xj[c].y - (Real)xi[a].y, dz = (Real)xj[c].z - (Real)xi[a].z;
                    const Real r2 = noe_fma(dz, dz, noe_fma(dy, dy, dx * dx));
                    const Real ri = noe_rsqrt(r2);
                    const Real ri2 = ri * ri, ri3 = ri2 * ri, ri5 = ri3 * ri2, ri6 = ri3 * ri3;
                    Real px = dx, py = dy, pz = dz;
                    if (ROT) {
                        px = noe_fma(R[0], dx, noe_fma(R[1], dy, R[2] * dz));
                        py = noe_fma(R[4], dx, noe_fma(R[5], dy, R[6] * dz));
                        pz = noe_fma(R[8], dx, noe_fma(R[9], dy, R[10] * dz));
                    }
                    const Real sx = px * ri5, sy = py * ri5, sz = pz * ri5;
                    Real *A = acc[a][c];
                    A[0] += ri6;
                    A[1] = noe_fma(sx, px, A[1]);
                    A[2] = noe_fma(sy, py, A[2]);
                    A[3] = noe_fma(sz, pz, A[3]);
                    A[4] = noe_fma(sx, py, A[4]);
                    A[5] = noe_fma(sx, pz, A[5]);
                    A[6] = noe_fma(sy, pz, A[6]);
                }
            if ((f & (kFlush - 1)) == kFlush - 1) flush();
        }
        if (nf & (kFlush - 1)) flush();                    // a short last stage that ended between two flushes
    }

    // S > 1: a partial tile, (row, column, 7), row = position in tile ti, column = position in tile tj;
    // S = 1: the pairs i < j < P straight into sums[b] (of a diagonal tile's skipped quarter every pair has i >= j)
    double *out = S > 1 ? part + ((int64_t)(b * S + s) * NP + p) * kPart : sums + (int64_t)b * npairs * 7;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int r = ty + 16 * a, q = tx + 16 * c;
            const int64_t i = (int64_t)ti * kTile + r, j = (int64_t)tj * kTile + q;
            if (S == 1 && (i >= j || j >= P)) continue;
            double *o = out + (S > 1 ? (int64_t)(r * kTile + q) : i * (2 * (int64_t)P - i - 1) / 2 + (j - i - 1)) * 7;
#pragma unroll
            for (int k = 0; k < 7; ++k) o[k] = sizeof(Real) == sizeof(double) ? (double)acc[a][c][k] : tot[a][c][k];
        }
}

__global__ __launch_bounds__(256) void k_noe_finish(const double *__restrict__ part, int P, int nT, int NP, int S, int64_t npairs,
                                                    double *__restrict__ sums)
{
    const int p = blockIdx.x, b = blockIdx.y;
    int ti, tj;
    noe_tile_pair(p, nT, ti, tj);
    const double *src = part + ((int64_t)b * S * NP + p) * kPart;
    double *dst = sums + (int64_t)b * npairs * 7;
    const int e = blockIdx.z * 256 + threadIdx.x;         // one value of the tile per thread: kPart / 256 = 28 workgroups per tile
    const int pr = e / 7, k = e - 7 * pr, r = pr / kTile, c = pr - r * kTile;
    const int64_t i = (int64_t)ti * kTile + r, j = (int64_t)tj * kTile + c;
    if (i >= P || j >= P || i >= j) return;
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += src[(int64_t)s * NP * kPart + e];
    dst[(i * (2 * (int64_t)P - i - 1) / 2 + (j - i - 1)) * 7 + k] = sum;
}

}  // namespace

// everything that is refused, before anything is queued
int noe_check(sr_ctx *ctx, const char *who, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const int64_t *bs,
              const int64_t *bl, int B, int mode, NoeShape &sh)
{
    SR_REQUIRE(nFrames >= 1 && nAtoms >= 1, -3, "%s: bad shape nFrames=%lld nAtoms=%lld", who, (long long)nFrames, (long long)nAtoms);
    SR_REQUIRE(P >= 2, -3, "%s: P=%lld atoms; a pair needs two", who, (long long)P);
    SR_REQUIRE(P <= nAtoms && P <= ((int64_t)1 << 20), -3, "%s: P=%lld distinct atoms of %lld (at most 2^20)", who, (long long)P, (long long)nAtoms);
    SR_REQUIRE(mode == 0 || mode == 1, -3, "%s: mode %d (0: float32, 1: float64)", who, mode);
    SR_REQUIRE(B >= 1, -3, "%s: B=%d frame blocks", who, B);
    std::vector<char> seen((size_t)nAtoms, 0);
    for (int64_t k = 0; k < P; ++k) {
        SR_REQUIRE(index[k] >= 0 && index[k] < nAtoms, -3, "%s: index[%lld] = %d is outside the %lld atoms", who, (long long)k, (int)index[k],
                   (long long)nAtoms);
        SR_REQUIRE(!seen[index[k]], -3, "%s: index[%lld] = %d is listed twice", who, (long long)k, (int)index[k]);
        seen[index[k]] = 1;
    }
    sh.Fmax = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t a = bs[b], n = bl[b];
        SR_REQUIRE(n >= 1, -3, "%s: block %d has length %lld", who, b, (long long)n);
        SR_REQUIRE(a >= 0 && a <= nFrames && n <= nFrames - a, -3, "%s: block %d = frames [%lld, %lld) is outside the %lld held", who, b,
                   (long long)a, (long long)(a + n), (long long)nFrames);
        if (n > sh.Fmax) sh.Fmax = n;
    }
    sh.nT = (P + kTile - 1) / kTile;
    sh.NP = sh.nT * (sh.nT + 1) / 2;
    sh.npairs = P * (P - 1) / 2;
    sh.S = noe_ksplit(sh.NP, sh.Fmax, B);
    // P <= 2^20: npairs < 2^39, NP < 2^29, so the products below stay inside 128 bits by a wide margin
    const unsigned __int128 out_bytes = (unsigned __int128)B * (unsigned __int128)sh.npairs * 56u;
    const unsigned __int128 part_bytes =
        sh.S > 1 ? (unsigned __int128)B * (unsigned __int128)sh.S * (unsigned __int128)sh.NP * (kPart * sizeof(double)) : 0;
    const unsigned __int128 have = ctx->prop.totalGlobalMem;
    SR_REQUIRE(out_bytes <= have && part_bytes <= have && out_bytes + part_bytes <= have, -3,
               "%s: %d blocks x %lld pairs x 56 bytes = %.1f GiB of sums (and %.1f GiB of partial tiles) do not fit the device's %.1f GiB", who, B,
               (long long)sh.npairs, (double)out_bytes / 1073741824.0, (double)part_bytes / 1073741824.0, (double)have / 1073741824.0);
    SR_REQUIRE((unsigned __int128)B * sh.S * sh.NP < ((unsigned __int128)1 << 31) && B <= 65535 && sh.NP < ((int64_t)1 << 31), -3,
               "%s: %lld tile pairs x %d splits x %d blocks are too many for one call", who, (long long)sh.NP, sh.S, B);
    return 0;
}

extern "C" {

int sr_noe_tile(void) { return kTile; }
int sr_noe_frame_batch(void) { return kFB; }

int sr_noe_pairs_check(sr_ctx *ctx, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const int64_t *block_start,
                       const int64_t *block_len, int B, int mode)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(index && block_start && block_len, -2, "sr_noe_pairs_check: null pointer");
    NoeShape sh;
    return noe_check(ctx, "sr_noe_pairs_check", nFrames, nAtoms, index, P, block_start, block_len, B, mode, sh);
}

int sr_noe_pairs_f32_dev(sr_ctx *ctx, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index_host, int64_t P,
                         const double *quat, const int64_t *block_start_host, const int64_t *block_len_host, int B, int mode, double *sums)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(xyz && index_host && block_start_host && block_len_host && sums, -2, "sr_noe_pairs_f32_dev: null pointer");
    NoeShape sh;
    if (int rc = noe_check(ctx, "sr_noe_pairs_f32_dev", nFrames, nAtoms, index_host, P, block_start_host, block_len_host, B, mode, sh)) return rc;
    // ---- the block table, (start, length) pairs, then the atom indices; the partial tiles ----
    const size_t tab_bytes = (size_t)B * 2 * sizeof(int64_t);
    char *misc = (char *)sr_workspace(ctx, SR_WS_MISC, tab_bytes + (size_t)P * sizeof(int));
    double *part = sh.S > 1 ? (double *)sr_workspace(ctx, SR_WS_NOE, (size_t)B * sh.S * sh.NP * kPart * sizeof(double)) : nullptr;
    if (!misc || (sh.S > 1 && !part)) return -5;
    int64_t *blk_dev = (int64_t *)misc;
    int *idx_dev = (int *)(misc + tab_bytes);
    std::vector<int64_t> table((size_t)B * 2);
    for (int b = 0; b < B; ++b) { table[2 * b] = block_start_host[b]; table[2 * b + 1] = block_len_host[b]; }
    SR_HIP(hipMemcpyAsync(blk_dev, table.data(), tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    SR_HIP(hipMemcpyAsync(idx_dev, index_host, (size_t)P * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    SR_HIP(hipStreamSynchronize(ctx->stream));          // small tables: the caller's arrays are free again when this returns
    // ---- launch ----
    const dim3 grid((unsigned)((int64_t)B * sh.S * sh.NP)), block(256);
    int rc;
#define NOE_LAUNCH(Real, ROT)                                                                                                       \
    sr_launch(ctx, k_noe_pairs<Real, ROT>, grid, block, 0, xyz, nAtoms, (const int *)idx_dev, (int)P, quat, (const int64_t *)blk_dev, \
              (int)sh.nT, (int)sh.NP, sh.S, part, sums, sh.npairs)
    if (mode == 0) rc = quat ? NOE_LAUNCH(float, true) : NOE_LAUNCH(float, false);
    else rc = quat ? NOE_LAUNCH(double, true) : NOE_LAUNCH(double, false);
#undef NOE_LAUNCH
    if (rc || sh.S == 1) return rc;
    return sr_launch(ctx, k_noe_finish, dim3((unsigned)sh.NP, (unsigned)B, kPart / 256), dim3(256), 0, (const double *)part, (int)P, (int)sh.nT, (int)sh.NP,
                     sh.S, sh.npairs, sums);
}

int sr_noe_pairs_f32(sr_ctx *ctx, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const double *quat,
                     const int64_t *block_start, const int64_t *block_len, int B, int mode, double *sums)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(xyz && index && block_start && block_len && sums, -2, "sr_noe_pairs_f32: null pointer");
    NoeShape sh;
    if (int rc = noe_check(ctx, "sr_noe_pairs_f32", nFrames, nAtoms, index, P, block_start, block_len, B, mode, sh)) return rc;
    const size_t nin = (size_t)nFrames * nAtoms * 3, nq = (size_t)nFrames * 4, nout = (size_t)B * sh.npairs * 7;
    sr_stage st(ctx);
    const float *xyz_d = st.open(SR_WS_VECS, nin * sizeof(float)).put(xyz, nin);
    const double *q_d = quat ? st.open(SR_WS_IN0, nq * sizeof(double)).put(quat, nq) : nullptr;
    double *sums_d = st.take<double>(SR_WS_OUT0, nout);
    if (st.rc) return st.rc;
    if (int rc = sr_noe_pairs_f32_dev(ctx, xyz_d, nFrames, nAtoms, index, P, q_d, block_start, block_len, B, mode, sums_d)) return rc;
    st.fetch(sums, sums_d, nout);
    return st.finish();
}

}  // extern "C"
