// sr_noe_host.h -- the pure host arithmetic of the all-pairs dipolar map, its lagged form and the lagged form's split into tumbling
// modes (sr_noe.hip): split rule, lag list check, origin ranges, byte counts, grid sizes, quaternion and frame matrix.  Nothing here
// needs HIP: scripts/dev/noe_lagged_host_sweep.cpp compiles this header alone, with -fsanitize=address,undefined, and sweeps it.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>

#ifdef __HIPCC__
#define SR_NOE_HD __host__ __device__ __forceinline__
#else
#define SR_NOE_HD inline
#endif

constexpr int kNoeTile = 32;                        // atoms per tile side
constexpr int kNoeMaxLags = 64;                     // lags per call of the lagged map
constexpr int kNoeLagPart = kNoeTile * kNoeTile;    // pairs of a tile: float64 values of one sum of one partial tile
constexpr int kNoeMapSums = 7;                      // sums per (block, pair) of the map: r^-6 and the six tensor components
constexpr int kNoeModeSums = 6;                     // sums per (block, lag, pair) of the mode-resolved map: H0 .. H5

// the split rule: a function of the shape alone: about sixteen workgroups per CU of a 256-CU part (three fit a SIMD at a time: several
// rounds of them keep the last round short), each with at least 128 frames, at most 256 partial tiles to add
inline int noe_ksplit(int64_t NP, int64_t Fmax, int B)
{
    int64_t S = (4096 + NP * B - 1) / (NP * B);
    const int64_t by_frames = Fmax / 128 > 1 ? Fmax / 128 : 1;
    if (S > by_frames) S = by_frames;
    if (S > 256) S = 256;
    return (int)S;
}

// ---- the lagged map ----
// The lags of a call: 1 .. kNoeMaxLags of them, >= 0, strictly increasing, the largest below the shortest block (every (block, lag)
// has at least one term).  0, or -3 with the reason in msg.
inline int noe_lag_check(const int32_t *lags, int K, int64_t shortest, char *msg, size_t nmsg)
{
    if (K < 1 || K > kNoeMaxLags) {
        snprintf(msg, nmsg, "K=%d lags (1 .. %d)", K, kNoeMaxLags);
        return -3;
    }
    for (int q = 0; q < K; ++q) {
        if (lags[q] < 0) {
            snprintf(msg, nmsg, "lag[%d] = %d is negative", q, (int)lags[q]);
            return -3;
        }
        if (q > 0 && lags[q] <= lags[q - 1]) {
            snprintf(msg, nmsg, "lags must be strictly increasing: lag[%d] = %d after %d", q, (int)lags[q], (int)lags[q - 1]);
            return -3;
        }
    }
    if (lags[K - 1] >= shortest) {
        snprintf(msg, nmsg, "lag %d leaves no term in a block of %lld frames", (int)lags[K - 1], (long long)shortest);
        return -3;
    }
    return 0;
}

// the origins t - start that split s < S owns of a block of len frames at lag k < len: runs of ceil((len - k) / S) of the len - k
// origins; the second window of a split reads up to k frames past hi, never past len
SR_NOE_HD void noe_lag_origins(int64_t len, int64_t k, int S, int s, int64_t &lo, int64_t &hi)
{
    const int64_t no = len - k;
    const int64_t per = (no + S - 1) / S;
    lo = (int64_t)s * per;
    hi = lo + per;
    if (lo > no) lo = no;
    if (hi > no) hi = no;
}

// bytes of the result (B, K, npairs, M) float64 and of the partial tiles (B, K, S, NP, M, T x T) float64 (none with S = 1): the map is
// K = 1, M = 7, its lagged form M = 1, the mode-resolved form M = kNoeModeSums.
// P <= 2^20: npairs < 2^39, NP < 2^29, B < 2^31, K <= 64, S <= 256, M <= 7: inside 128 bits by a wide margin
inline void noe_bytes(int B, int K, int M, int64_t npairs, int S, int64_t NP, unsigned __int128 &out_bytes, unsigned __int128 &part_bytes)
{
    out_bytes = (unsigned __int128)B * (unsigned)K * (unsigned)M * (unsigned __int128)npairs * 8u;
    part_bytes = S > 1 ? (unsigned __int128)B * (unsigned)K * (unsigned)S * (unsigned)M * (unsigned __int128)NP * (kNoeLagPart * 8u) : 0;
}

// the tile kernels take B K S NP workgroups in one dimension, below 2^31.  4 B K NP was the grid of the lagged map's own finish
// kernel and stays a refusal; k_noe_finish (4 M B K NP workgroups) runs only with S > 1, that is B NP < 4096 (noe_ksplit)
inline bool noe_grid_ok(int B, int K, int S, int64_t NP)
{
    const unsigned __int128 bk = (unsigned __int128)B * (unsigned)K * (unsigned __int128)NP, lim = (unsigned __int128)1 << 31;
    return bk * (unsigned)S < lim && bk * 4u < lim;
}

// the unit quaternion (w, x, y, z) -> R(q), row-major 3 x 3 in float64, each entry as written: no contraction
SR_NOE_HD void noe_quat_matrix(double w, double x, double y, double z, double *A)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    A[0] = 1 - 2 * (y * y + z * z); A[1] = 2 * (x * y - w * z);     A[2] = 2 * (x * z + w * y);
    A[3] = 2 * (x * y + w * z);     A[4] = 1 - 2 * (x * x + z * z); A[5] = 2 * (y * z - w * x);
    A[6] = 2 * (x * z - w * y);     A[7] = 2 * (y * z + w * x);     A[8] = 1 - 2 * (x * x + y * y);
}

// the frame quaternion (w, x, y, z) -> F = R(q / |q|), row-major 3 x 3 in float64; 0, or -3 with the reason in msg: a component that
// is not finite, a squared norm farther than 1e-6 from 1.  NULL: the identity.
inline int noe_frame_matrix(const double *q, double *F, char *msg, size_t nmsg)
{
    for (int k = 0; k < 9; ++k) F[k] = (k % 4 == 0) ? 1.0 : 0.0;
    if (!q) return 0;
    double n2 = 0.0;
    for (int k = 0; k < 4; ++k) {
        if (!(q[k] - q[k] == 0.0)) {                // NaN or infinite
            snprintf(msg, nmsg, "frame quaternion component %d = %g is not finite", k, q[k]);
            return -3;
        }
        n2 += q[k] * q[k];
    }
    if (!(n2 >= 1.0 - 1e-6 && n2 <= 1.0 + 1e-6)) {
        snprintf(msg, nmsg, "frame quaternion of squared norm %.9g is not a unit quaternion", n2);
        return -3;
    }
    const double n = 1.0 / std::sqrt(n2);
    noe_quat_matrix(q[0] * n, q[1] * n, q[2] * n, q[3] * n, F);
    return 0;
}
