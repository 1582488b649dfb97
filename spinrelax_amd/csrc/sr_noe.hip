// sr_noe.hip -- the all-pairs dipolar map, the map at a few chosen lags and the lagged map split into tumbling modes: three sets of sums
// per frame block b = frames [s, s + n) and per pair i < j of P selected atoms, with d = x_j - x_i of the raw float32 coordinates,
// r = |d| and d'(t) = R(q_t) d(t), each frame with its own quaternion.  The loops of the domain that are quadratic in the number of
// spins; unlike the iRED matrix they are non-linear per pair and frame (a reciprocal square root and its powers): vector ALU work,
// nothing for the matrix pipe.  The three kernels are one workgroup body (sr_noe_tile.h: tiles, staging, splits, epilogue, the shared
// head of the arithmetic) with a term each, and one host path (noe_check, noe_run, noe_entry below).
//
// k_noe_pairs, the map (Brueschweiler et al., JACS 1992; Peter, Daura & van Gunsteren, J. Biomol. NMR 2001): the sums over the block's
// frames of
//
//     r^-6     and     d'_a d'_b r^-5   (ab = xx, yy, zz, xy, xz, yz)
//
// <r^-6>, <r^-3> = tr T, the effective distances and the order parameters S2_ij = 1.5 (T:T - A3^2 / 3) / A6, S2_rad = A3^2 / A6 are host
// work (spinrelax_amd/noe.py).  About 30 instructions per pair and frame.  Into sums[b][pair][7].
//
// k_noe_lagged, per lag k:
//
//     G_b(k)_ij = sum_{t = s}^{s + n - k - 1} [1.5 (d'(t) . d'(t + k))^2 / (r(t)^2 r(t + k)^2) - 0.5] r(t)^-3 r(t + k)^-3
//
// The rotation does not cancel as it does in r.  G_b(0) is the map's r^-6 sum; C_dd(k) = [sum_b G_b(k) / sum_b (n_b - k)] / <r^-6> and the
// per-pair internal correlation time from it are host work (spinrelax_amd/noe.py).  Into G[b][k][pair].
//
// k_noe_modes, per lag k, the five tumbling modes of an anisotropic rotational diffusion tensor: the six sums
//
//     H0 = sum w qz(u) qz(v)        H1 = sum w dl(u) dl(v)        H2 = sum w [qz(u) dl(v) + dl(u) qz(v)] / 2
//     H3 = sum w uy uz vy vz        H4 = sum w ux uz vx vz        H5 = sum w ux uy vx vy
//
// over the origins t = s .. s + n - k - 1, with d"(t) = F R(q_t) d(t) (F = R(q_F) the constant rotation into the tensor's principal-axis
// frame), u = d"(t) / r(t), v = d"(t + k) / r(t + k), w = r(t)^-3 r(t + k)^-3, qz(u) = uz^2 - 1/3 and dl(u) = ux^2 - uy^2.  The sums do not
// depend on the tensor; the amplitudes of its five modes are linear in them (spinrelax_amd/noe.py: mode_amplitudes).  With
// Q = u u^T - 1/3: P2(u . v) = 1.5 Q : Q' = 2.25 qz qz' + 0.75 dl dl' + 3 (uy uz vy vz + ux uz vx vz + ux uy vx vy), so that
// 2.25 H0 + 0.75 H1 + 3 (H3 + H4 + H5) = G of k_noe_lagged, whatever F.  Into H[b][k][pair][6].
//
// The split count of all three is noe_ksplit(tile pairs, longest block, B) -- the map's own, WITHOUT the number of lags: what a
//   workgroup adds, and in which order, then depends on its own (block, lag, split) alone, and the value of a lag has the same bits alone
//   and in any list.  (With B K in the place of B the splits, and the last bits, of a lag would move with the number of lags asked for
//   beside it.)
#include "sr_noe_tile.h"
#include <vector>

namespace {

// Each term: the operation sequence behind the body's d', ri (sr_noe_tile.h), explicit and without contraction, in Real = float (mode 0)
// or double (mode 1); p = d'(t), ri = 1 / r(t); with two windows q = d'(t + k) and si = 1 / r(t + k) as well.
struct NoeRotation {                        // what the map and the lagged map store per frame: R = Real(R(q) in float64)
    static __device__ __forceinline__ bool quat_given(const double *) { return true; }
    template <typename Real>
    __device__ __forceinline__ void matrix(const double *q, Real *R) const
    {
        double A[9];
        noe_quat_matrix(q[0], q[1], q[2], q[3], A);
#pragma unroll
        for (int k = 0; k < 9; ++k) R[4 * (k / 3) + k % 3] = (Real)A[k];
    }
};

//       ri2  = ri * ri,  ri3 = ri2 * ri,  ri5 = ri3 * ri2,  ri6 = ri3 * ri3
//       s_a  = p_a * ri5;   sums: += ri6, fma(s_a, p_b, .)
struct NoePairsTerm : NoeRotation {
    static constexpr int kWindows = 1, kSums = kNoeMapSums;
    static __host__ __device__ constexpr int64_t part_offset(int m, int64_t n) { return n * kSums + m; }
    static __host__ __device__ constexpr void part_place(int e, int &m, int &n) { n = e / kSums; m = e - n * kSums; }
    template <bool ROT, typename Real>
    static __device__ __forceinline__ void add(Real *A, const Real (&d)[1][3], const Real (&rv)[1], const Real (&M)[1][12])
    {
#pragma clang fp contract(off)
        const Real ri = rv[0];
        const Real ri2 = ri * ri, ri3 = ri2 * ri, ri5 = ri3 * ri2, ri6 = ri3 * ri3;
        Real p[3];
        noe_rotate<ROT>(M[0], d[0], p);                 // behind the powers of 1 / r, as the sequence has it
        const Real px = p[0], py = p[1], pz = p[2];
        const Real sx = px * ri5, sy = py * ri5, sz = pz * ri5;
        A[0] += ri6;
        A[1] = noe_fma(sx, px, A[1]);
        A[2] = noe_fma(sy, py, A[2]);
        A[3] = noe_fma(sz, pz, A[3]);
        A[4] = noe_fma(sx, py, A[4]);
        A[5] = noe_fma(sx, pz, A[5]);
        A[6] = noe_fma(sy, pz, A[6]);
    }
};

//       c    = fma(pz, qz, fma(py, qy, px * qx))
//       g    = ri * si;  x = c * g;  g3 = (g * g) * g
//       p2   = fma(1.5 * x, x, -0.5);  term = p2 * g3
struct NoeLaggedTerm : NoeRotation {
    static constexpr int kWindows = 2, kSums = 1;
    static __host__ __device__ constexpr int64_t part_offset(int m, int64_t n) { return m * kNoeLagPart + n; }
    static __host__ __device__ constexpr void part_place(int e, int &m, int &n) { m = e / kNoeLagPart; n = e - m * kNoeLagPart; }
    template <bool ROT, typename Real>
    static __device__ __forceinline__ void add(Real *A, const Real (&d)[2][3], const Real (&rv)[2], const Real (&M)[2][12])
    {
#pragma clang fp contract(off)
        Real pv[2][3];
        noe_rotate<ROT>(M[0], d[0], pv[0]);
        noe_rotate<ROT>(M[1], d[1], pv[1]);
        const Real cc = noe_fma(pv[0][2], pv[1][2], noe_fma(pv[0][1], pv[1][1], pv[0][0] * pv[1][0]));
        const Real g = rv[0] * rv[1];
        const Real x = cc * g;
        const Real g3 = (g * g) * g;
        const Real pp = noe_fma((Real)1.5 * x, x, (Real)-0.5);
        A[0] += pp * g3;
    }
};

struct FrameMat {
    double m[9];                            // F, row-major
};

// The quaternion threads compose F into their frame's matrix, M = Real(F R(q_t) in float64), rounded once; without quaternions
// R(q_t) = 1 and the matrix is F; without either the no-rotation instantiation runs.
//       u_a  = p_a * ri,  v_a = q_a * si
//       a0   = fma(uz, uz, -1/3),  a1 = fma(ux, ux, -(uy * uy));  b0, b1 of v likewise
//       g    = ri * si;  g3 = (g * g) * g
//       t0 = (a0 * b0) * g3;  t1 = (a1 * b1) * g3;  t2 = (0.5 * fma(a0, b1, a1 * b0)) * g3
//       t3 = ((uy * uz) * (vy * vz)) * g3;  t4 = ((ux * uz) * (vx * vz)) * g3;  t5 = ((ux * uy) * (vx * vy)) * g3
struct NoeModesTerm {
    static constexpr int kWindows = 2, kSums = kNoeModeSums;
    FrameMat F;
    static __device__ __forceinline__ bool quat_given(const double *quat) { return quat != nullptr; }
    static __host__ __device__ constexpr int64_t part_offset(int m, int64_t n) { return m * kNoeLagPart + n; }
    static __host__ __device__ constexpr void part_place(int e, int &m, int &n) { m = e / kNoeLagPart; n = e - m * kNoeLagPart; }
    template <typename Real>
    __device__ __forceinline__ void matrix(const double *q, Real *R) const
    {
#pragma clang fp contract(off)
        double A[9];
        noe_quat_matrix(q[0], q[1], q[2], q[3], A);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                R[4 * r + c] = (Real)__builtin_fma(F.m[3 * r + 2], A[6 + c], __builtin_fma(F.m[3 * r + 1], A[3 + c], F.m[3 * r] * A[c]));
    }
    template <bool ROT, typename Real>
    static __device__ __forceinline__ void add(Real *A, const Real (&d)[2][3], const Real (&rv)[2], const Real (&M)[2][12])
    {
#pragma clang fp contract(off)
        Real pv[2][3];
        noe_rotate<ROT>(M[0], d[0], pv[0]);
        noe_rotate<ROT>(M[1], d[1], pv[1]);
        const Real ri = rv[0], si = rv[1];
        const Real ux = pv[0][0] * ri, uy = pv[0][1] * ri, uz = pv[0][2] * ri;
        const Real vx = pv[1][0] * si, vy = pv[1][1] * si, vz = pv[1][2] * si;
        const Real third = (Real)(-1.0 / 3.0);
        const Real a0 = noe_fma(uz, uz, third), a1 = noe_fma(ux, ux, -(uy * uy));
        const Real b0 = noe_fma(vz, vz, third), b1 = noe_fma(vx, vx, -(vy * vy));
        const Real g = ri * si;
        const Real g3 = (g * g) * g;
        A[0] += (a0 * b0) * g3;
        A[1] += (a1 * b1) * g3;
        A[2] += ((Real)0.5 * noe_fma(a0, b1, a1 * b0)) * g3;
        A[3] += ((uy * uz) * (vy * vz)) * g3;
        A[4] += ((ux * uz) * (vx * vz)) * g3;
        A[5] += ((ux * uy) * (vx * vy)) * g3;
    }
};

template <typename Real, bool ROT>
__global__ __launch_bounds__(256) void k_noe_pairs(const float *__restrict__ xyz, int64_t nAtoms, const int *__restrict__ index, int P,
                                                   const double *__restrict__ quat, const int64_t *__restrict__ blk, int nT, int NP, int S,
                                                   double *__restrict__ part, double *__restrict__ sums, int64_t npairs)
{
    noe_tile_body<NoePairsTerm, Real, ROT>(NoePairsTerm{}, xyz, nAtoms, index, P, quat, blk, nullptr, 1, nT, NP, S, part, sums, npairs);
}

template <typename Real, bool ROT>
__global__ __launch_bounds__(256) void k_noe_lagged(const float *__restrict__ xyz, int64_t nAtoms, const int *__restrict__ index, int P,
                                                    const double *__restrict__ quat, const int64_t *__restrict__ blk,
                                                    const int *__restrict__ lags, int K, int nT, int NP, int S, double *__restrict__ part,
                                                    double *__restrict__ G, int64_t npairs)
{
    noe_tile_body<NoeLaggedTerm, Real, ROT>(NoeLaggedTerm{}, xyz, nAtoms, index, P, quat, blk, lags, K, nT, NP, S, part, G, npairs);
}

template <typename Real, bool ROT>
__global__ __launch_bounds__(256) void k_noe_modes(const float *__restrict__ xyz, int64_t nAtoms, const int *__restrict__ index, int P,
                                                   const double *__restrict__ quat, FrameMat F, const int64_t *__restrict__ blk,
                                                   const int *__restrict__ lags, int K, int nT, int NP, int S, double *__restrict__ part,
                                                   double *__restrict__ H, int64_t npairs)
{
    noe_tile_body<NoeModesTerm, Real, ROT>(NoeModesTerm{F}, xyz, nAtoms, index, P, quat, blk, lags, K, nT, NP, S, part, H, npairs);
}

// ---- the host path of the nine entry points ----
enum { NOE_PAIRS, NOE_LAGGED, NOE_MODES };     // NoeCall::kind
enum { NOE_CHECK, NOE_DEV, NOE_HOST };         // what an entry point is: the refusals alone; xyz, quat and out on the device; on the host

struct NoeCall {
    int kind;
    const float *xyz;
    int64_t nFrames, nAtoms;
    const int32_t *index;
    int64_t P;
    const double *quat, *frame_quat;
    const int64_t *bs, *bl;
    int B;
    const int32_t *lags;
    int K, mode;
    double *out;
    int sums() const { return kind == NOE_PAIRS ? kNoeMapSums : kind == NOE_LAGGED ? 1 : kNoeModeSums; }
};

struct NoeShape {
    int64_t nT, NP, npairs, Fmax;
    int S;
    FrameMat F;
};

// everything that is refused, before anything is queued: the map's refusals, its memory and grid included, for every kind; then the
// lags, the frame quaternion, the memory and the grid of the lagged kinds.  Fills sh.
int noe_check(sr_ctx *ctx, const char *who, const NoeCall &c, NoeShape &sh)
{
    const int64_t nFrames = c.nFrames, nAtoms = c.nAtoms, P = c.P;
    const int B = c.B, K = c.K;
    SR_REQUIRE(nFrames >= 1 && nAtoms >= 1, -3, "%s: bad shape nFrames=%lld nAtoms=%lld", who, (long long)nFrames, (long long)nAtoms);
    SR_REQUIRE(P >= 2, -3, "%s: P=%lld atoms; a pair needs two", who, (long long)P);
    SR_REQUIRE(P <= nAtoms && P <= ((int64_t)1 << 20), -3, "%s: P=%lld distinct atoms of %lld (at most 2^20)", who, (long long)P, (long long)nAtoms);
    SR_REQUIRE(c.mode == 0 || c.mode == 1, -3, "%s: mode %d (0: float32, 1: float64)", who, c.mode);
    SR_REQUIRE(B >= 1, -3, "%s: B=%d frame blocks", who, B);
    std::vector<char> seen((size_t)nAtoms, 0);
    for (int64_t k = 0; k < P; ++k) {
        SR_REQUIRE(c.index[k] >= 0 && c.index[k] < nAtoms, -3, "%s: index[%lld] = %d is outside the %lld atoms", who, (long long)k, (int)c.index[k],
                   (long long)nAtoms);
        SR_REQUIRE(!seen[c.index[k]], -3, "%s: index[%lld] = %d is listed twice", who, (long long)k, (int)c.index[k]);
        seen[c.index[k]] = 1;
    }
    sh.Fmax = 0;
    int64_t shortest = c.bl[0];
    for (int b = 0; b < B; ++b) {
        const int64_t a = c.bs[b], n = c.bl[b];
        SR_REQUIRE(n >= 1, -3, "%s: block %d has length %lld", who, b, (long long)n);
        SR_REQUIRE(a >= 0 && a <= nFrames && n <= nFrames - a, -3, "%s: block %d = frames [%lld, %lld) is outside the %lld held", who, b,
                   (long long)a, (long long)(a + n), (long long)nFrames);
        if (n > sh.Fmax) sh.Fmax = n;
        if (n < shortest) shortest = n;
    }
    sh.nT = (P + kTile - 1) / kTile;
    sh.NP = sh.nT * (sh.nT + 1) / 2;
    sh.npairs = P * (P - 1) / 2;
    sh.S = noe_ksplit(sh.NP, sh.Fmax, B);
    const unsigned __int128 have = ctx->prop.totalGlobalMem;
    unsigned __int128 out_bytes, part_bytes;
    noe_bytes(B, 1, kNoeMapSums, sh.npairs, sh.S, sh.NP, out_bytes, part_bytes);
    SR_REQUIRE(out_bytes <= have && part_bytes <= have && out_bytes + part_bytes <= have, -3,
               "%s: %d blocks x %lld pairs x 56 bytes = %.1f GiB of sums (and %.1f GiB of partial tiles) do not fit the device's %.1f GiB", who, B,
               (long long)sh.npairs, (double)out_bytes / 1073741824.0, (double)part_bytes / 1073741824.0, (double)have / 1073741824.0);
    // B <= 65535 dates from the map's own finish kernel, whose grid had the blocks in y; k_noe_finish no longer needs it, the refusal
    // stays.  noe_grid_ok adds 4 B NP < 2^31 to what the map refused before; it cannot be reached: B NP >= 2^29 with B <= 65535 is
    // 2^13 and more tile pairs, tens of terabytes of sums, which the memory check above has refused
    SR_REQUIRE(noe_grid_ok(B, 1, sh.S, sh.NP) && B <= 65535 && sh.NP < ((int64_t)1 << 31), -3,
               "%s: %lld tile pairs x %d splits x %d blocks are too many for one call", who, (long long)sh.NP, sh.S, B);
    if (c.kind == NOE_PAIRS) return 0;
    char msg[160];
    int rc = noe_lag_check(c.lags, K, shortest, msg, sizeof msg);
    if (!rc && c.kind == NOE_MODES) rc = noe_frame_matrix(c.frame_quat, sh.F.m, msg, sizeof msg);
    if (rc) {
        sr_set_error("%s: %s", who, msg);
        return rc;
    }
    noe_bytes(B, K, c.sums(), sh.npairs, sh.S, sh.NP, out_bytes, part_bytes);
    SR_REQUIRE(out_bytes <= have && part_bytes <= have && out_bytes + part_bytes <= have, -3,
               "%s: %d blocks x %d lags x %lld pairs x %s8 bytes = %.1f GiB of %s (and %.1f GiB of partial tiles) do not fit the device's %.1f GiB", who,
               B, K, (long long)sh.npairs, c.kind == NOE_MODES ? "6 x " : "", (double)out_bytes / 1073741824.0, c.kind == NOE_MODES ? "H" : "G",
               (double)part_bytes / 1073741824.0, (double)have / 1073741824.0);
    SR_REQUIRE(noe_grid_ok(B, K, sh.S, sh.NP), -3, "%s: %lld tile pairs x %d splits x %d lags x %d blocks are too many for one call", who,
               (long long)sh.NP, sh.S, K, B);
    return 0;
}

// a checked call with xyz, quat and out on the device: the small tables, the kernel of (kind, mode, rotation), the finish
int noe_run(sr_ctx *ctx, const NoeCall &c, const NoeShape &sh)
{
    const int B = c.B, K = c.kind == NOE_PAIRS ? 1 : c.K, P = (int)c.P, nT = (int)sh.nT, NP = (int)sh.NP, S = sh.S;
    // ---- the block table, (start, length) pairs, then the atom indices and the lags; the partial tiles ----
    const size_t tab_bytes = (size_t)B * 2 * sizeof(int64_t), nlag = c.kind == NOE_PAIRS ? 0 : (size_t)K;
    char *misc = (char *)sr_workspace(ctx, SR_WS_MISC, tab_bytes + ((size_t)P + nlag) * sizeof(int));
    double *part = S > 1 ? (double *)sr_workspace(ctx, SR_WS_NOE, (size_t)B * K * S * NP * c.sums() * kNoeLagPart * sizeof(double)) : nullptr;
    if (!misc || (S > 1 && !part)) return -5;
    const int64_t *blk = (const int64_t *)misc;
    const int *idx = (const int *)(misc + tab_bytes), *lag = idx + P;
    std::vector<int64_t> table((size_t)B * 2);
    for (int b = 0; b < B; ++b) { table[2 * b] = c.bs[b]; table[2 * b + 1] = c.bl[b]; }
    SR_HIP(hipMemcpyAsync(misc, table.data(), tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    SR_HIP(hipMemcpyAsync(misc + tab_bytes, c.index, (size_t)P * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    if (nlag) SR_HIP(hipMemcpyAsync(misc + tab_bytes + (size_t)P * sizeof(int), c.lags, nlag * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    SR_HIP(hipStreamSynchronize(ctx->stream));          // small tables: the caller's arrays are free again when this returns
    // ---- launch ----
    const dim3 grid((unsigned)((int64_t)B * K * S * NP)), block(256);
    const bool rotate = c.quat || (c.kind == NOE_MODES && c.frame_quat);
#define NOE_PICK(LAUNCH) \
    (c.mode == 0 ? (rotate ? LAUNCH(float, true) : LAUNCH(float, false)) : (rotate ? LAUNCH(double, true) : LAUNCH(double, false)))
#define NOE_LAUNCH_PAIRS(Real, ROT) \
    sr_launch(ctx, k_noe_pairs<Real, ROT>, grid, block, 0, c.xyz, c.nAtoms, idx, P, c.quat, blk, nT, NP, S, part, c.out, sh.npairs)
#define NOE_LAUNCH_LAGGED(Real, ROT) \
    sr_launch(ctx, k_noe_lagged<Real, ROT>, grid, block, 0, c.xyz, c.nAtoms, idx, P, c.quat, blk, lag, K, nT, NP, S, part, c.out, sh.npairs)
#define NOE_LAUNCH_MODES(Real, ROT) \
    sr_launch(ctx, k_noe_modes<Real, ROT>, grid, block, 0, c.xyz, c.nAtoms, idx, P, c.quat, sh.F, blk, lag, K, nT, NP, S, part, c.out, sh.npairs)
    const int rc = c.kind == NOE_PAIRS ? NOE_PICK(NOE_LAUNCH_PAIRS) : c.kind == NOE_LAGGED ? NOE_PICK(NOE_LAUNCH_LAGGED) : NOE_PICK(NOE_LAUNCH_MODES);
#undef NOE_LAUNCH_MODES
#undef NOE_LAUNCH_LAGGED
#undef NOE_LAUNCH_PAIRS
#undef NOE_PICK
    if (rc || S == 1) return rc;
    const auto finish = c.kind == NOE_PAIRS ? k_noe_finish<NoePairsTerm> : c.kind == NOE_LAGGED ? k_noe_finish<NoeLaggedTerm> : k_noe_finish<NoeModesTerm>;
    // S > 1 means B NP < 4096 (noe_ksplit): at most 64 lags x 28 workgroups each, far below the grid limit
    return sr_launch(ctx, finish, dim3((unsigned)((int64_t)B * K * NP * (c.sums() * kNoeLagPart / 256))), dim3(256), 0, (const double *)part, P, nT,
                     NP, S, sh.npairs, c.out);
}

// an entry point: null pointers (-2), the refusals (-3), then nothing more (NOE_CHECK), the run on the caller's device arrays (NOE_DEV)
// or on staged copies of the caller's host arrays (NOE_HOST)
int noe_entry(sr_ctx *ctx, const char *who, int what, NoeCall c)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(c.index && c.bs && c.bl && (c.kind == NOE_PAIRS || c.lags || c.K < 1) && (what == NOE_CHECK || (c.xyz && c.out)), -2,
               "%s: null pointer", who);
    NoeShape sh;
    if (int rc = noe_check(ctx, who, c, sh)) return rc;
    if (what == NOE_CHECK) return 0;
    if (what == NOE_DEV) return noe_run(ctx, c, sh);
    const size_t nin = (size_t)c.nFrames * c.nAtoms * 3, nq = (size_t)c.nFrames * 4;
    const size_t nout = (size_t)c.B * (c.kind == NOE_PAIRS ? 1 : c.K) * sh.npairs * c.sums();
    double *out_host = c.out;
    sr_stage st(ctx);
    c.xyz = st.open(SR_WS_VECS, nin * sizeof(float)).put(c.xyz, nin);
    c.quat = c.quat ? st.open(SR_WS_IN0, nq * sizeof(double)).put(c.quat, nq) : nullptr;
    c.out = st.take<double>(SR_WS_OUT0, nout);
    if (st.rc) return st.rc;
    if (int rc = noe_run(ctx, c, sh)) return rc;
    st.fetch(out_host, c.out, nout);
    return st.finish();
}

}  // namespace

extern "C" {

int sr_noe_tile(void) { return kTile; }
int sr_noe_frame_batch(void) { return kFB; }

int sr_noe_lagged_splits(int64_t P, int64_t longest_block, int B)
{
    if (P < 2 || longest_block < 1 || B < 1) return 0;
    const int64_t nT = (P + kTile - 1) / kTile;
    return noe_ksplit(nT * (nT + 1) / 2, longest_block, B);
}

int sr_noe_pairs_check(sr_ctx *ctx, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const int64_t *block_start,
                       const int64_t *block_len, int B, int mode)
{
    return noe_entry(ctx, "sr_noe_pairs_check", NOE_CHECK,
                     {NOE_PAIRS, nullptr, nFrames, nAtoms, index, P, nullptr, nullptr, block_start, block_len, B, nullptr, 1, mode, nullptr});
}

int sr_noe_pairs_f32_dev(sr_ctx *ctx, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index_host, int64_t P,
                         const double *quat, const int64_t *block_start_host, const int64_t *block_len_host, int B, int mode, double *sums)
{
    return noe_entry(ctx, "sr_noe_pairs_f32_dev", NOE_DEV,
                     {NOE_PAIRS, xyz, nFrames, nAtoms, index_host, P, quat, nullptr, block_start_host, block_len_host, B, nullptr, 1, mode, sums});
}

int sr_noe_pairs_f32(sr_ctx *ctx, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const double *quat,
                     const int64_t *block_start, const int64_t *block_len, int B, int mode, double *sums)
{
    return noe_entry(ctx, "sr_noe_pairs_f32", NOE_HOST,
                     {NOE_PAIRS, xyz, nFrames, nAtoms, index, P, quat, nullptr, block_start, block_len, B, nullptr, 1, mode, sums});
}

int sr_noe_lagged_check(sr_ctx *ctx, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const int64_t *block_start,
                        const int64_t *block_len, int B, const int32_t *lags, int K, int mode)
{
    return noe_entry(ctx, "sr_noe_lagged_check", NOE_CHECK,
                     {NOE_LAGGED, nullptr, nFrames, nAtoms, index, P, nullptr, nullptr, block_start, block_len, B, lags, K, mode, nullptr});
}

int sr_noe_lagged_f32_dev(sr_ctx *ctx, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index_host, int64_t P,
                          const double *quat, const int64_t *block_start_host, const int64_t *block_len_host, int B,
                          const int32_t *lags_host, int K, int mode, double *G)
{
    return noe_entry(ctx, "sr_noe_lagged_f32_dev", NOE_DEV,
                     {NOE_LAGGED, xyz, nFrames, nAtoms, index_host, P, quat, nullptr, block_start_host, block_len_host, B, lags_host, K, mode, G});
}

int sr_noe_lagged_f32(sr_ctx *ctx, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const double *quat,
                      const int64_t *block_start, const int64_t *block_len, int B, const int32_t *lags, int K, int mode, double *G)
{
    return noe_entry(ctx, "sr_noe_lagged_f32", NOE_HOST,
                     {NOE_LAGGED, xyz, nFrames, nAtoms, index, P, quat, nullptr, block_start, block_len, B, lags, K, mode, G});
}

int sr_noe_modes_check(sr_ctx *ctx, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const int64_t *block_start,
                       const int64_t *block_len, int B, const int32_t *lags, int K, const double *frame_quat, int mode)
{
    return noe_entry(ctx, "sr_noe_modes_check", NOE_CHECK,
                     {NOE_MODES, nullptr, nFrames, nAtoms, index, P, nullptr, frame_quat, block_start, block_len, B, lags, K, mode, nullptr});
}

int sr_noe_modes_f32_dev(sr_ctx *ctx, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index_host, int64_t P,
                         const double *quat, const double *frame_quat_host, const int64_t *block_start_host, const int64_t *block_len_host,
                         int B, const int32_t *lags_host, int K, int mode, double *H)
{
    return noe_entry(ctx, "sr_noe_modes_f32_dev", NOE_DEV, {NOE_MODES, xyz, nFrames, nAtoms, index_host, P, quat, frame_quat_host,
                                                            block_start_host, block_len_host, B, lags_host, K, mode, H});
}

int sr_noe_modes_f32(sr_ctx *ctx, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const double *quat,
                     const double *frame_quat, const int64_t *block_start, const int64_t *block_len, int B, const int32_t *lags, int K, int mode,
                     double *H)
{
    return noe_entry(ctx, "sr_noe_modes_f32", NOE_HOST,
                     {NOE_MODES, xyz, nFrames, nAtoms, index, P, quat, frame_quat, block_start, block_len, B, lags, K, mode, H});
}

}  // extern "C"
