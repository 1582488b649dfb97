// sr_noesy.hip -- NOESY intensities from the all-pairs dipolar map by the full relaxation matrix (Macura & Ernst, Mol. Phys. 41, 95
// (1980); Keepers & James, J. Magn. Reson. 57, 404 (1984); model-free rates: Brueschweiler et al., JACS 114, 2289 (1992)):
//
//     R_ij = sigma_ij = q A6 [6 J(2w) - J(0)]                     A(tau_m) = exp(-R tau_m)
//     R_ii = sum_j q A6 [J(0) + 3 J(w) + 6 J(2w)] + leak_i        J(w) = S2 tc / (1 + w^2 tc^2) + (1 - S2) t' / (1 + w^2 t'^2)
//
// with 1 / t' = 1 / tc + 1 / te, A6 = <r^-6> and S2 of the map (sr_noe.hip, spinrelax_amd/noe.py), q = prefactor (0.1 (mu0 / 4 pi)^2
// hbar^2 gamma_H^4 in units of the coordinates).  Isotropic tumbling, one kind of spin.
//
// k_noesy_rates: one workgroup per row i.  Thread t computes the pairs (i, j), j = t, t + 256, ..., from A6 / S2 / tau_e at
//   pair_index(min, max): sigma_ij and sigma_ji come from the same values by the same instructions, so R is exactly symmetric.  The
//   thread's rho_ij are added in the order of j, the 256 partial sums by a tree in LDS: a fixed order, no atomics.  S2 is clipped
//   to [0, 1].
//
// k_symm_mul: C = alpha A B + beta I for symmetric A and B that commute (every matrix below is a polynomial in R): the product is
//   symmetric, so only the tiles with tile row <= tile column are computed -- half the flops of a general product.  A tile is
//   C[I, J] = sum_K A[I, K] B[J, K]^T: both operands are read as ROWS (B[K, J] = B[J, K]), contiguous along k.
//   One workgroup (4 waves) per (tile pair, k split); a tile is 64 x 64, a wave owns a 32 x 32 quarter as 2 x 2 accumulators of
//   v_mfma_f64_16x16x4_f64: the layout of k_ired_matrix (sr_ired.hip), lane l gives A[row l & 15][k = l >> 4] and
//   B[col l & 15][k = l >> 4]; accumulator col = lane & 15, row = (lane >> 4) + 4 reg.
//   LDS holds kK = 32 columns of the 64 + 64 rows as float64, [side][row][kLD = 34]: the 16 rows x 2 k of the 32 lanes that share an
//   LDS cycle of a ds_read_b64 lie at dwords 2 (34 r + k) = 4 r + 2 k mod 64 -- 32 different bank pairs.  The next stage is fetched
//   into registers (16 float64 per thread) while the current one is multiplied.  Rows past P and columns past the split's range are
//   staged as zeros, which add exactly 0.
//   For symmetric input that does not commute the result is DEFINED as: the tiles with tile row <= tile column of alpha A B + beta I
//   (of a diagonal tile the entries i <= j), mirrored below.
// k_symm_mul_finish: one workgroup per 16 x 16 block of a tile, one value per thread: adds the S partial tiles of a tile pair in the
//   order s = 0 .. S-1, applies alpha and beta and writes C[i][j] and C[j][i] from one value, the mirror image through a 16 x 16
//   transpose in LDS so that both are written along rows.  No atomics: equal input gives equal bits and C == C^T bit for bit.  It
//   runs behind every workgroup of k_symm_mul, so C may be A or B.
// S is a function of P alone: min(64, max(1, P / 64), ceil(1024 / tile pairs)); split s owns the columns [s per, (s + 1) per),
//   per = ceil(P / S) rounded up to whole stages.
//
// sr_symm_expm_f64_dev: out[k] = exp(-R tau_k) by scaling and squaring: X = R tau, s = the least integer >= 0 with
//   |X|_1 / 2^s <= kTheta = 0.5, Y = -X / 2^s, p = sum_{n <= 12} Y^n / n! by Horner (11 products), then s squarings, every product by
//   k_symm_mul.  Each mixing time is computed from R on its own: A(tau) has the same bits alone and in a list.
#include "sr_internal.h"
#include <cmath>
#include <vector>

namespace {

constexpr int kTile = 64;                   // rows per tile side
constexpr int kK = 32;                      // columns of k per LDS stage: a multiple of 4 (one MFMA k-step)
constexpr int kLD = kK + 2;                 // LDS row pitch in float64: kLD / 2 odd (banks, see above)
constexpr int kStage = 2 * kTile * kK;      // float64 values per stage
constexpr int kPerThread = kStage / 256;    // 16
constexpr int kMaxP = 32768;
constexpr double kTheta = 0.5;              // scaling: |Y|_1 <= kTheta
constexpr int kDegree = 12;                 // Taylor degree: kTheta^13 / 13! = 2e-14 relative to the last kept term's scale
static_assert(kK % 4 == 0 && (kLD / 2) % 2 == 1 && kLD % 2 == 0 && kStage % 256 == 0 && 256 % kK == 0, "stage shape");

typedef double d4 __attribute__((ext_vector_type(4)));

// tile pair p = 0 .. T (T + 1) / 2 - 1, row-major over ti <= tj
__device__ __forceinline__ void symm_pair(int p, int T, int &ti, int &tj)
{
    ti = 0;
    while (p >= T - ti) { p -= T - ti; ++ti; }
    tj = ti + p;
}

// sum of one value per thread of a 256-thread workgroup in a fixed order (a tree in LDS); the total in every thread
__device__ __forceinline__ double block_sum_256(double v, double *red)
{
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    const double tot = red[0];
    __syncthreads();
    return tot;
}

__device__ __forceinline__ double noesy_J(double w, double S2, double tc, double tp)
{
    return S2 * tc / (1.0 + w * w * tc * tc) + (1.0 - S2) * tp / (1.0 + w * w * tp * tp);
}

__global__ __launch_bounds__(256) void k_noesy_rates(const double *__restrict__ A6, const double *__restrict__ S2, const double *__restrict__ tau_e,
                                                     const double *__restrict__ leak, int P, double omega, double tau_c, double tau_e_all,
                                                     double leak_all, double q, double *__restrict__ R)
{
#pragma clang fp contract(off)
    __shared__ double red[256];
    const int i = blockIdx.x;
    double rho = 0.0;
    for (int j = threadIdx.x; j < P; j += 256) {
        if (j == i) continue;
        const int64_t a = i < j ? i : j, b = i < j ? j : i;
        const int64_t k = a * (2 * (int64_t)P - a - 1) / 2 + (b - a - 1);
        double s2 = S2[k];
        s2 = s2 < 0.0 ? 0.0 : (s2 > 1.0 ? 1.0 : s2);
        const double te = tau_e ? tau_e[k] : tau_e_all;
        const double tp = tau_c * te / (tau_c + te);
        const double J0 = noesy_J(0.0, s2, tau_c, tp), J1 = noesy_J(omega, s2, tau_c, tp), J2 = noesy_J(2.0 * omega, s2, tau_c, tp);
        const double qa = q * A6[k];
        R[(int64_t)i * P + j] = qa * (6.0 * J2 - J0);
        rho += qa * (J0 + 3.0 * J1 + 6.0 * J2);
    }
    const double tot = block_sum_256(rho, red);
    if (threadIdx.x == 0) R[(int64_t)i * P + i] = tot + (leak ? leak[i] : leak_all);
}

struct ModeRates {
    double E[5];                            // the tensor's five rates, the order of _hostmath.D_coefficients_ellipsoid
};

__device__ __forceinline__ double noesy_g(double x, double y) { return x / (x * x + y * y); }      // as in sr_relax.hip

// anisotropic tumbling: per pair the amplitudes a[k][m] of the five modes at lag 0 and their plateaus c[k][m], both in units of A6.
// tau_e per (pair, mode), per pair or one for all.  The structure of k_noesy_rates: the same row sum, R_ij and R_ji from one value.
__global__ __launch_bounds__(256) void k_noesy_rates_modes(const double *__restrict__ am, const double *__restrict__ cm,
                                                           const double *__restrict__ tau_e_pair, const double *__restrict__ tau_e_mode,
                                                           const double *__restrict__ leak, int P, double omega, ModeRates rates,
                                                           double tau_e_all, double leak_all, double q, double *__restrict__ R)
{
#pragma clang fp contract(off)
    __shared__ double red[256];
    const int i = blockIdx.x;
    double rho = 0.0;
    for (int j = threadIdx.x; j < P; j += 256) {
        if (j == i) continue;
        const int64_t a = i < j ? i : j, b = i < j ? j : i;
        const int64_t k = a * (2 * (int64_t)P - a - 1) / 2 + (b - a - 1);
        const double te = tau_e_pair ? tau_e_pair[k] : tau_e_all;
        double J0 = 0.0, J1 = 0.0, J2 = 0.0;
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            const double c = cm[5 * k + m];
            double d = am[5 * k + m] - c;
            d = d > 0.0 ? d : 0.0;
            const double E = rates.E[m], Ef = E + 1.0 / (tau_e_mode ? tau_e_mode[5 * k + m] : te);
            J0 += c * noesy_g(E, 0.0) + d * noesy_g(Ef, 0.0);
            J1 += c * noesy_g(E, omega) + d * noesy_g(Ef, omega);
            J2 += c * noesy_g(E, 2.0 * omega) + d * noesy_g(Ef, 2.0 * omega);
        }
        R[(int64_t)i * P + j] = q * (6.0 * J2 - J0);
        rho += q * (J0 + 3.0 * J1 + 6.0 * J2);
    }
    const double tot = block_sum_256(rho, red);
    if (threadIdx.x == 0) R[(int64_t)i * P + i] = tot + (leak ? leak[i] : leak_all);
}

// sums[i] = sum_j |R_ij|, in a fixed order: a non-finite entry makes its row's sum non-finite
__global__ __launch_bounds__(256) void k_symm_rowsum(const double *__restrict__ R, int P, double *__restrict__ sums)
{
    __shared__ double red[256];
    const int i = blockIdx.x;
    double v = 0.0;
    for (int j = threadIdx.x; j < P; j += 256) v += fabs(R[(int64_t)i * P + j]);
    const double tot = block_sum_256(v, red);
    if (threadIdx.x == 0) sums[i] = tot;
}

// Y = c R and the innermost Horner factor p = I + Y / kDegree
__global__ __launch_bounds__(256) void k_symm_expm_init(const double *__restrict__ R, int P, double c, double *__restrict__ Y, double *__restrict__ p)
{
    const int64_t n = (int64_t)P * P;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const double y = c * R[e];
        Y[e] = y;
        p[e] = y / (double)kDegree + ((e / P == e % P) ? 1.0 : 0.0);
    }
}

__global__ __launch_bounds__(256) void k_symm_mul(const double *__restrict__ A, const double *__restrict__ B, int P, int T, int NP, int64_t per,
                                                  double *__restrict__ part)
{
    __shared__ double lds[2 * kTile * kLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x % NP, s = blockIdx.x / NP;
    int ti, tj;
    symm_pair(p, T, ti, tj);
    const int64_t k0 = (int64_t)s * per < P ? (int64_t)s * per : P;
    const int64_t k1 = k0 + per < P ? k0 + per : P;

    // what this thread fetches of every stage: column kk of the staged rows (tid >> 5) + 8 q, q < 8 of A's tile row ti, the others
    // of B's tile row tj; null = a row past P
    const int kk = tid & (kK - 1);
    const double *src[kPerThread];
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
        const int row = (tid >> 5) + 8 * q, side = row / kTile, r = row - side * kTile;
        const int64_t g = (int64_t)(side ? tj : ti) * kTile + r;
        src[q] = g < P ? (side ? B : A) + g * P + kk : nullptr;
    }
    double pre[kPerThread];
    auto fetch = [&](int64_t ks) {
        const bool in = ks + kk < k1;
#pragma unroll
        for (int q = 0; q < kPerThread; ++q) pre[q] = (src[q] && in) ? src[q][ks] : 0.0;
    };

    d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};

    // this lane's operand sources: row (lane & 15) of each of the wave's two 16-row groups of either side, column lane >> 4
    const int wr = wave >> 1, wc = wave & 1, lv = lane & 15, lk = lane >> 4;
    const double *rowp[2], *colp[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        rowp[g] = lds + (0 * kTile + wr * 32 + g * 16 + lv) * kLD + lk;
        colp[g] = lds + (1 * kTile + wc * 32 + g * 16 + lv) * kLD + lk;
    }

    if (k0 < k1) fetch(k0);
    for (int64_t ks = k0; ks < k1; ks += kK) {
        __syncthreads();                                   // the previous stage has been read
#pragma unroll
        for (int q = 0; q < kPerThread; ++q) lds[((tid >> 5) + 8 * q) * kLD + kk] = pre[q];
        __syncthreads();
        if (ks + kK < k1) fetch(ks + kK);                  // in flight during the products below
        const int steps = (int)((k1 - ks < kK ? k1 - ks : (int64_t)kK) + 3) / 4;
        for (int k = 0; k < steps; ++k) {
            double a[2], b[2];
#pragma unroll
            for (int g = 0; g < 2; ++g) { a[g] = rowp[g][4 * k]; b[g] = colp[g][4 * k]; }
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b[y], acc[x][y], 0, 0, 0);
        }
    }

    // partial tile, row-major 64 x 64; f64 accumulator map: col = lane & 15, row = (lane >> 4) + 4 reg
    double *out = part + ((int64_t)s * NP + p) * (kTile * kTile);
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

__global__ __launch_bounds__(256) void k_symm_mul_finish(const double *__restrict__ part, int P, int T, int NP, int S, double alpha, double beta,
                                                         double *__restrict__ C)
{
    __shared__ double tr[16][17];
    const int p = blockIdx.x, br = blockIdx.y >> 2, bc = blockIdx.y & 3;       // one 16 x 16 block of the tile per workgroup
    int ti, tj;
    symm_pair(p, T, ti, tj);
    if (ti == tj && br > bc) return;                       // wholly below the diagonal
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int r = br * 16 + ty, c = bc * 16 + tx, e = r * kTile + c;
    const double *src = part + (int64_t)p * (kTile * kTile) + e;
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += src[(int64_t)s * NP * (kTile * kTile)];
    const int64_t i = (int64_t)ti * kTile + r, j = (int64_t)tj * kTile + c;
    const double m = alpha * sum + (i == j ? beta : 0.0);
    if (i < P && j < P && !(ti == tj && r > c)) C[i * P + j] = m;
    // the mirror image from the same value, through LDS so that it too is written along rows
    tr[ty][tx] = m;
    __syncthreads();
    const int r2 = br * 16 + tx, c2 = bc * 16 + ty;
    const int64_t i2 = (int64_t)ti * kTile + r2, j2 = (int64_t)tj * kTile + c2;
    if (i2 < P && j2 < P && !(ti == tj && r2 >= c2)) C[j2 * P + i2] = tr[tx][ty];
}

struct SymmShape {
    int64_t T, NP, per;
    int S;
    size_t part_bytes;
};

// the split rule: a function of P alone (never of the device or of a timing): about four workgroups per CU of a 256-CU part, each
// with at least 64 columns, at most 64 partial tiles to add
SymmShape symm_shape(int64_t P)
{
    SymmShape sh;
    sh.T = (P + kTile - 1) / kTile;
    sh.NP = sh.T * (sh.T + 1) / 2;
    int64_t S = (1024 + sh.NP - 1) / sh.NP;
    const int64_t by_k = P / 64 > 1 ? P / 64 : 1;
    if (S > by_k) S = by_k;
    if (S > 64) S = 64;
    sh.S = (int)S;
    sh.per = sr_round_up((P + S - 1) / S, kK);
    sh.part_bytes = (size_t)(sh.NP * S) * kTile * kTile * sizeof(double);
    return sh;
}

// both kernels of one product, queued on ctx->stream; part holds sh.part_bytes
int symm_mul_launch(sr_ctx *ctx, const SymmShape &sh, const double *A, const double *B, int64_t P, double alpha, double beta, double *part, double *C)
{
    if (int rc = sr_launch(ctx, k_symm_mul, dim3((unsigned)(sh.NP * sh.S)), dim3(256), 0, A, B, (int)P, (int)sh.T, (int)sh.NP, sh.per, part)) return rc;
    return sr_launch(ctx, k_symm_mul_finish, dim3((unsigned)sh.NP, 16), dim3(256), 0, (const double *)part, (int)P, (int)sh.T, (int)sh.NP, sh.S, alpha,
                     beta, C);
}

// the scaling of one mixing time: the least s >= 0 with norm1 tau / 2^s <= kTheta (exact: a power of two scales without rounding)
int expm_plan(const char *who, double norm1, double tau, int *s_out, int *products)
{
    SR_REQUIRE(std::isfinite(norm1) && norm1 >= 0.0, -3, "%s: |R|_1 = %g: R is not finite", who, norm1);
    SR_REQUIRE(std::isfinite(tau) && tau >= 0.0, -3, "%s: mixing time %g (finite and >= 0)", who, tau);
    const double x = norm1 * tau;
    SR_REQUIRE(std::isfinite(x), -3, "%s: |R|_1 tau = %g x %g is not finite", who, norm1, tau);
    int s = 0;
    while (s <= 40 && std::ldexp(x, -s) > kTheta) ++s;
    SR_REQUIRE(s <= 40, -3, "%s: |R|_1 tau = %g needs more than 40 squarings", who, x);
    if (s_out) *s_out = s;
    if (products) *products = kDegree - 1 + s;
    return 0;
}

// the sizes of one exponential call, and the refusal of what cannot fit: out + work area against the device's memory, and the part
// of the work area that the context does not hold yet (with `with_out` the outputs too) against the memory that is free now
int expm_memory(sr_ctx *ctx, const char *who, int64_t P, int64_t n_tau, bool with_out, SymmShape &sh, size_t &y_bytes)
{
    SR_REQUIRE(P >= 1 && P <= kMaxP, -3, "%s: P=%lld (1 .. %d)", who, (long long)P, kMaxP);
    SR_REQUIRE(n_tau >= 1 && n_tau <= 65536, -3, "%s: %lld mixing times (1 .. 65536)", who, (long long)n_tau);
    sh = symm_shape(P);
    y_bytes = (size_t)P * P * sizeof(double) + (size_t)P * sizeof(double);          // Y, then the row sums
    const double GiB = 1073741824.0;
    const unsigned __int128 out_bytes = (unsigned __int128)n_tau * (unsigned __int128)P * (unsigned __int128)P * 8u;
    const unsigned __int128 ws_bytes = (unsigned __int128)y_bytes + sh.part_bytes;
    SR_REQUIRE(out_bytes + ws_bytes <= (unsigned __int128)ctx->prop.totalGlobalMem, -3,
               "%s: %lld x %lld x %lld x 8 bytes = %.2f GiB of results and %.2f GiB of work area do not fit the device's %.2f GiB", who,
               (long long)n_tau, (long long)P, (long long)P, (double)out_bytes / GiB, (double)ws_bytes / GiB, (double)ctx->prop.totalGlobalMem / GiB);
    size_t free_b = 0, total_b = 0;
    SR_HIP(hipMemGetInfo(&free_b, &total_b));
    unsigned __int128 need = with_out ? out_bytes : 0;
    // what sr_workspace would allocate (12.5 % head-room); a slot that grows is freed first
    unsigned __int128 have = free_b;
    if (ctx->slot_bytes[SR_WS_EXPM] < y_bytes) { need += y_bytes + y_bytes / 8; have += ctx->slot_bytes[SR_WS_EXPM]; }
    if (ctx->slot_bytes[SR_WS_SYMM] < sh.part_bytes) { need += sh.part_bytes + sh.part_bytes / 8; have += ctx->slot_bytes[SR_WS_SYMM]; }
    SR_REQUIRE(need <= have, -3, "%s: %.2f GiB to allocate (%s%.2f GiB of work area for P=%lld) but %.2f GiB of device memory are free", who,
               (double)need / GiB, with_out ? "results and " : "", (double)ws_bytes / GiB, (long long)P, (double)have / GiB);
    return 0;
}

// what the rate entry points refuse, before anything is queued
int rates_check(const char *who, const double *A6, const double *S2, const double *tau_e, const double *leak, int64_t P, double omega, double tau_c,
                double tau_e_all, double leak_all, double q)
{
    SR_REQUIRE(P >= 2, -3, "%s: P=%lld spins; a pair needs two", who, (long long)P);
    SR_REQUIRE(P <= kMaxP, -3, "%s: P=%lld spins; at most %d", who, (long long)P, kMaxP);
    SR_REQUIRE(std::isfinite(omega) && omega >= 0.0, -3, "%s: omega_H = %g rad/s", who, omega);
    SR_REQUIRE(std::isfinite(tau_c) && tau_c > 0.0, -3, "%s: tau_c = %g (finite and > 0)", who, tau_c);
    SR_REQUIRE(std::isfinite(q) && q > 0.0, -3, "%s: prefactor %g (finite and > 0)", who, q);
    if (!tau_e) SR_REQUIRE(std::isfinite(tau_e_all) && tau_e_all > 0.0, -3, "%s: tau_e = %g (finite and > 0)", who, tau_e_all);
    if (!leak) SR_REQUIRE(std::isfinite(leak_all) && leak_all >= 0.0, -3, "%s: leak = %g (finite and >= 0)", who, leak_all);
    const int64_t np = P * (P - 1) / 2;
    for (int64_t k = 0; k < np; ++k) {
        SR_REQUIRE(std::isfinite(A6[k]) && A6[k] > 0.0, -3, "%s: A6[%lld] = %g (finite and > 0)", who, (long long)k, A6[k]);
        SR_REQUIRE(S2[k] >= -1e-6 && S2[k] <= 1.0 + 1e-6, -3, "%s: S2[%lld] = %.17g is outside [0, 1]", who, (long long)k, S2[k]);
        if (tau_e) SR_REQUIRE(std::isfinite(tau_e[k]) && tau_e[k] > 0.0, -3, "%s: tau_e[%lld] = %g (finite and > 0)", who, (long long)k, tau_e[k]);
    }
    if (leak)
        for (int64_t i = 0; i < P; ++i)
            SR_REQUIRE(std::isfinite(leak[i]) && leak[i] >= 0.0, -3, "%s: leak[%lld] = %g (finite and >= 0)", who, (long long)i, leak[i]);
    return 0;
}

// stages the pair and spin arrays (one slot) and queues k_noesy_rates; the caller waits before the host arrays change
int rates_run(sr_ctx *ctx, sr_stage &st, const double *A6, const double *S2, const double *tau_e, const double *leak, int64_t P, double omega,
              double tau_c, double tau_e_all, double leak_all, double q, double *R_dev)
{
    const size_t np = (size_t)(P * (P - 1) / 2);
    st.open(SR_WS_IN0, ((tau_e ? 3 : 2) * np + (size_t)P) * sizeof(double));
    const double *a6_d = st.put(A6, np), *s2_d = st.put(S2, np), *te_d = st.put(tau_e, np), *lk_d = st.put(leak, (size_t)P);
    if (st.rc) return st.rc;
    return sr_launch(ctx, k_noesy_rates, dim3((unsigned)P), dim3(256), 0, a6_d, s2_d, te_d, lk_d, (int)P, omega, tau_c, tau_e_all, leak_all, q, R_dev);
}

// what the mode-resolved rate entry points refuse, before anything is queued
int rates_modes_check(sr_ctx *ctx, const char *who, const double *a, const double *c, const double *E, const double *tau_e_pair,
                      const double *tau_e_mode, const double *leak, int64_t P, double omega, double tau_e_all, double leak_all, double q)
{
    SR_REQUIRE(P >= 2, -3, "%s: P=%lld spins; a pair needs two", who, (long long)P);
    SR_REQUIRE(P <= kMaxP, -3, "%s: P=%lld spins; at most %d", who, (long long)P, kMaxP);
    const int64_t np = P * (P - 1) / 2;
    // the staged tables (a, c, tau_e) and R: P <= 32768, below 2^40 bytes
    const uint64_t bytes = ((uint64_t)np * (10 + (tau_e_mode ? 5 : 0) + (tau_e_pair ? 1 : 0)) + (uint64_t)P + (uint64_t)P * P) * 8u;
    SR_REQUIRE(bytes <= (uint64_t)ctx->prop.totalGlobalMem, -3, "%s: the tables of %lld pairs and R, %.2f GiB, do not fit the device's %.2f GiB", who,
               (long long)np, (double)bytes / 1073741824.0, (double)ctx->prop.totalGlobalMem / 1073741824.0);
    SR_REQUIRE(std::isfinite(omega) && omega >= 0.0, -3, "%s: omega_H = %g rad/s", who, omega);
    SR_REQUIRE(std::isfinite(q) && q > 0.0, -3, "%s: prefactor %g (finite and > 0)", who, q);
    for (int m = 0; m < 5; ++m) SR_REQUIRE(std::isfinite(E[m]) && E[m] > 0.0, -3, "%s: E[%d] = %g (finite and > 0)", who, m, E[m]);
    if (!tau_e_pair && !tau_e_mode) SR_REQUIRE(std::isfinite(tau_e_all) && tau_e_all > 0.0, -3, "%s: tau_e = %g (finite and > 0)", who, tau_e_all);
    if (!leak) SR_REQUIRE(std::isfinite(leak_all) && leak_all >= 0.0, -3, "%s: leak = %g (finite and >= 0)", who, leak_all);
    for (int64_t k = 0; k < np; ++k) {
        for (int m = 0; m < 5; ++m) {
            const double am = a[5 * k + m], cm = c[5 * k + m];
            SR_REQUIRE(std::isfinite(am) && am >= 0.0, -3, "%s: a[%lld][%d] = %g (finite and >= 0)", who, (long long)k, m, am);
            SR_REQUIRE(std::isfinite(cm) && cm >= 0.0, -3, "%s: c[%lld][%d] = %g (finite and >= 0)", who, (long long)k, m, cm);
            SR_REQUIRE(cm <= am * (1.0 + 1e-6), -3, "%s: c[%lld][%d] = %.17g is above a = %.17g: a plateau lies below its function's start", who,
                       (long long)k, m, cm, am);
            if (tau_e_mode)
                SR_REQUIRE(std::isfinite(tau_e_mode[5 * k + m]) && tau_e_mode[5 * k + m] > 0.0, -3, "%s: tau_e[%lld][%d] = %g (finite and > 0)", who,
                           (long long)k, m, tau_e_mode[5 * k + m]);
        }
        if (tau_e_pair && !tau_e_mode)
            SR_REQUIRE(std::isfinite(tau_e_pair[k]) && tau_e_pair[k] > 0.0, -3, "%s: tau_e[%lld] = %g (finite and > 0)", who, (long long)k, tau_e_pair[k]);
    }
    if (leak)
        for (int64_t i = 0; i < P; ++i)
            SR_REQUIRE(std::isfinite(leak[i]) && leak[i] >= 0.0, -3, "%s: leak[%lld] = %g (finite and >= 0)", who, (long long)i, leak[i]);
    return 0;
}

// stages the pair and spin arrays (one slot) and queues k_noesy_rates_modes; the caller waits before the host arrays change
int rates_modes_run(sr_ctx *ctx, sr_stage &st, const double *a, const double *c, const double *E, const double *tau_e_pair, const double *tau_e_mode,
                    const double *leak, int64_t P, double omega, double tau_e_all, double leak_all, double q, double *R_dev)
{
    const size_t np = (size_t)(P * (P - 1) / 2);
    if (tau_e_mode) tau_e_pair = nullptr;               // the finer table wins
    st.open(SR_WS_IN0, ((10 + (tau_e_mode ? 5 : 0) + (tau_e_pair ? 1 : 0)) * np + (size_t)P) * sizeof(double));
    const double *a_d = st.put(a, 5 * np), *c_d = st.put(c, 5 * np), *tp_d = st.put(tau_e_pair, np), *tm_d = st.put(tau_e_mode, 5 * np),
                 *lk_d = st.put(leak, (size_t)P);
    if (st.rc) return st.rc;
    ModeRates rates;
    for (int m = 0; m < 5; ++m) rates.E[m] = E[m];
    return sr_launch(ctx, k_noesy_rates_modes, dim3((unsigned)P), dim3(256), 0, a_d, c_d, tp_d, tm_d, lk_d, (int)P, omega, rates, tau_e_all, leak_all, q,
                     R_dev);
}

}  // namespace

extern "C" {

int sr_noesy_rates_modes_f64_dev(sr_ctx *ctx, const double *a_host, const double *c_host, const double *E_host, const double *tau_e_pair_host,
                                 const double *tau_e_mode_host, const double *leak_host, int64_t P, double omega_H, double tau_e, double leak,
                                 double prefactor, double *R_dev)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(a_host && c_host && E_host && R_dev, -2, "sr_noesy_rates_modes_f64_dev: null pointer");
    if (int rc = rates_modes_check(ctx, "sr_noesy_rates_modes_f64_dev", a_host, c_host, E_host, tau_e_pair_host, tau_e_mode_host, leak_host, P, omega_H,
                                   tau_e, leak, prefactor))
        return rc;
    sr_stage st(ctx);
    if (int rc = rates_modes_run(ctx, st, a_host, c_host, E_host, tau_e_pair_host, tau_e_mode_host, leak_host, P, omega_H, tau_e, leak, prefactor, R_dev))
        return rc;
    return st.finish();                                 // the caller's arrays are free again when this returns
}

int sr_noesy_rates_modes_f64(sr_ctx *ctx, const double *a, const double *c, const double *E, const double *tau_e_pair, const double *tau_e_mode,
                             const double *leak_spin, int64_t P, double omega_H, double tau_e, double leak, double prefactor, double *R)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(a && c && E && R, -2, "sr_noesy_rates_modes_f64: null pointer");
    if (int rc = rates_modes_check(ctx, "sr_noesy_rates_modes_f64", a, c, E, tau_e_pair, tau_e_mode, leak_spin, P, omega_H, tau_e, leak, prefactor))
        return rc;
    sr_stage st(ctx);
    double *R_d = st.take<double>(SR_WS_OUT0, (size_t)P * P);
    if (st.rc) return st.rc;
    if (int rc = rates_modes_run(ctx, st, a, c, E, tau_e_pair, tau_e_mode, leak_spin, P, omega_H, tau_e, leak, prefactor, R_d)) return rc;
    st.fetch(R, R_d, (size_t)P * P);
    return st.finish();
}

int sr_noesy_rates_f64_dev(sr_ctx *ctx, const double *A6_host, const double *S2_host, const double *tau_e_host, const double *leak_host, int64_t P,
                           double omega_H, double tau_c, double tau_e, double leak, double prefactor, double *R_dev)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(A6_host && S2_host && R_dev, -2, "sr_noesy_rates_f64_dev: null pointer");
    if (int rc = rates_check("sr_noesy_rates_f64_dev", A6_host, S2_host, tau_e_host, leak_host, P, omega_H, tau_c, tau_e, leak, prefactor)) return rc;
    sr_stage st(ctx);
    if (int rc = rates_run(ctx, st, A6_host, S2_host, tau_e_host, leak_host, P, omega_H, tau_c, tau_e, leak, prefactor, R_dev)) return rc;
    return st.finish();                                 // the caller's arrays are free again when this returns
}

int sr_noesy_rates_f64(sr_ctx *ctx, const double *A6, const double *S2, const double *tau_e_pair, const double *leak_spin, int64_t P, double omega_H,
                       double tau_c, double tau_e, double leak, double prefactor, double *R)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(A6 && S2 && R, -2, "sr_noesy_rates_f64: null pointer");
    if (int rc = rates_check("sr_noesy_rates_f64", A6, S2, tau_e_pair, leak_spin, P, omega_H, tau_c, tau_e, leak, prefactor)) return rc;
    sr_stage st(ctx);
    double *R_d = st.take<double>(SR_WS_OUT0, (size_t)P * P);
    if (st.rc) return st.rc;
    if (int rc = rates_run(ctx, st, A6, S2, tau_e_pair, leak_spin, P, omega_H, tau_c, tau_e, leak, prefactor, R_d)) return rc;
    st.fetch(R, R_d, (size_t)P * P);
    return st.finish();
}

int sr_symm_mul_f64_dev(sr_ctx *ctx, const double *A, const double *B, int64_t P, double alpha, double beta, double *C)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(A && B && C, -2, "sr_symm_mul_f64_dev: null pointer");
    SR_REQUIRE(P >= 1 && P <= kMaxP, -3, "sr_symm_mul_f64_dev: P=%lld (1 .. %d)", (long long)P, kMaxP);
    SR_REQUIRE(std::isfinite(alpha) && std::isfinite(beta), -3, "sr_symm_mul_f64_dev: alpha = %g, beta = %g", alpha, beta);
    const SymmShape sh = symm_shape(P);
    double *part = (double *)sr_workspace(ctx, SR_WS_SYMM, sh.part_bytes);
    if (!part) return -5;
    return symm_mul_launch(ctx, sh, A, B, P, alpha, beta, part, C);
}

int sr_symm_expm_plan(double norm1, double tau, int *s, int *products) { return expm_plan("sr_symm_expm_plan", norm1, tau, s, products); }

int sr_symm_expm_check(sr_ctx *ctx, int64_t P, int64_t n_tau)
{
    SR_CHECK_CTX(ctx);
    SymmShape sh;
    size_t y_bytes;
    return expm_memory(ctx, "sr_symm_expm_check", P, n_tau, true, sh, y_bytes);
}

int sr_symm_expm_f64_dev(sr_ctx *ctx, const double *R, int64_t P, const double *tau_host, int64_t n_tau, double *out)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(R && tau_host && out, -2, "sr_symm_expm_f64_dev: null pointer");
    SymmShape sh;
    size_t y_bytes;
    if (int rc = expm_memory(ctx, "sr_symm_expm_f64_dev", P, n_tau, false, sh, y_bytes)) return rc;
    for (int64_t k = 0; k < n_tau; ++k)
        SR_REQUIRE(std::isfinite(tau_host[k]) && tau_host[k] >= 0.0, -3, "sr_symm_expm_f64_dev: mixing time %lld = %g (finite and >= 0)",
                   (long long)k, tau_host[k]);
    double *Y = (double *)sr_workspace(ctx, SR_WS_EXPM, y_bytes);
    double *part = (double *)sr_workspace(ctx, SR_WS_SYMM, sh.part_bytes);
    if (!Y || !part) return -5;
    // ---- |R|_1: row sums on the device (R is symmetric: rows = columns), their maximum here ----
    double *sums_d = Y + (size_t)P * P;
    if (int rc = sr_launch(ctx, k_symm_rowsum, dim3((unsigned)P), dim3(256), 0, R, (int)P, sums_d)) return rc;
    std::vector<double> sums((size_t)P);
    SR_HIP(hipMemcpyAsync(sums.data(), sums_d, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SR_HIP(hipStreamSynchronize(ctx->stream));
    double norm1 = 0.0;
    for (int64_t i = 0; i < P; ++i) norm1 = (sums[i] > norm1 || sums[i] != sums[i]) ? sums[i] : norm1;      // a NaN stays
    std::vector<int> sq((size_t)n_tau);
    for (int64_t k = 0; k < n_tau; ++k)
        if (int rc = expm_plan("sr_symm_expm_f64_dev", norm1, tau_host[k], &sq[k], nullptr)) return rc;
    // ---- every mixing time from R on its own ----
    const int64_t n = P * P;
    const unsigned init_grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    for (int64_t k = 0; k < n_tau; ++k) {
        double *p = out + k * n;
        const double c = -std::ldexp(tau_host[k], -sq[k]);
        if (int rc = sr_launch(ctx, k_symm_expm_init, dim3(init_grid), dim3(256), 0, R, (int)P, c, Y, p)) return rc;
        for (int m = kDegree - 1; m >= 1; --m)              // p = I + Y p / m
            if (int rc = symm_mul_launch(ctx, sh, Y, p, P, 1.0 / (double)m, 1.0, part, p)) return rc;
        for (int q = 0; q < sq[k]; ++q)
            if (int rc = symm_mul_launch(ctx, sh, p, p, P, 1.0, 0.0, part, p)) return rc;
    }
    return 0;
}

}  // extern "C"
