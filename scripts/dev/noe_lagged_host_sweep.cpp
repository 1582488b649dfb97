// Developer tool: sweeps the pure host helpers of the all-pairs dipolar map, its lagged and its mode-resolved form
// (spinrelax_amd/csrc/sr_noe_host.h: split rule, lag list check, origin ranges, byte counts, grid sizes, frame matrix) against plain
// restatements of their definitions, under the sanitizers.  No HIP, no GPU:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I spinrelax_amd/csrc \
//         scripts/dev/noe_lagged_host_sweep.cpp -o /tmp/noe_lagged_host_sweep && /tmp/noe_lagged_host_sweep
//
// Prints the number of comparisons and exits 0, or names the first disagreement and exits 1.
#include "sr_noe_host.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

static long checks = 0;
#define EXPECT(cond, ...)                                  \
    do {                                                   \
        ++checks;                                          \
        if (!(cond)) {                                     \
            fprintf(stderr, "FAILED %s: ", #cond);         \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                         \
            exit(1);                                       \
        }                                                  \
    } while (0)

int main()
{
    // ---- the split rule: min(256, max(1, Fmax / 128), ceil(4096 / (NP B))), never below 1 ----
    for (int64_t NP : std::initializer_list<int64_t>{1, 2, 3, 10, 136, 4095, 4096, 4097, (int64_t)1 << 28})
        for (int64_t F : std::initializer_list<int64_t>{1, 2, 127, 128, 255, 256, 300, 1000, 32768, 100000, (int64_t)1 << 40})
            for (int B : {1, 2, 3, 24, 65535}) {
                const int S = noe_ksplit(NP, F, B);
                int64_t want = (4096 + NP * B - 1) / (NP * B);
                if (want > (F / 128 > 1 ? F / 128 : 1)) want = F / 128 > 1 ? F / 128 : 1;
                if (want > 256) want = 256;
                EXPECT(S == want && S >= 1 && S <= 256, "noe_ksplit(%lld, %lld, %d) = %d", (long long)NP, (long long)F, B, S);
            }

    // ---- origin ranges: the S ranges tile [0, len - k) in order, none longer than ceil((len - k) / S), hi + k <= len ----
    for (int64_t len = 1; len <= 700; len += (len < 70 ? 1 : 37))
        for (int64_t k = 0; k < len; k += (k < 40 ? 1 : 29))
            for (int S : {1, 2, 3, 5, 7, 16, 255, 256}) {
                const int64_t no = len - k, per = (no + S - 1) / S;
                int64_t next = 0;
                for (int s = 0; s < S; ++s) {
                    int64_t lo, hi;
                    noe_lag_origins(len, k, S, s, lo, hi);
                    EXPECT(lo == next && hi >= lo && hi - lo <= per && hi + k <= len, "origins(len %lld, k %lld, S %d, s %d) = [%lld, %lld)",
                           (long long)len, (long long)k, S, s, (long long)lo, (long long)hi);
                    next = hi;
                }
                EXPECT(next == no, "origins(len %lld, k %lld, S %d) end at %lld", (long long)len, (long long)k, S, (long long)next);
            }
    // the map is lag 0: its frames in runs of ceil(len / S), [min(s per, len), min((s + 1) per, len))
    for (int64_t len = 1; len <= 700; len += (len < 70 ? 1 : 37))
        for (int S : {1, 2, 3, 5, 7, 16, 255, 256}) {
            const int64_t per = (len + S - 1) / S;
            for (int s = 0; s < S; ++s) {
                int64_t lo, hi;
                noe_lag_origins(len, 0, S, s, lo, hi);
                const int64_t a = (int64_t)s * per, b = a + per;
                EXPECT(lo == (a < len ? a : len) && hi == (b < len ? b : len), "map frames(len %lld, S %d, s %d) = [%lld, %lld)", (long long)len,
                       S, s, (long long)lo, (long long)hi);
            }
        }
    {   // at the largest values a call can carry
        int64_t lo, hi;
        noe_lag_origins(INT64_MAX / 512, 0, 256, 255, lo, hi);
        EXPECT(hi == INT64_MAX / 512 && lo <= hi, "origins at the largest block");
    }

    // ---- the lag list ----
    char msg[160];
    std::vector<int32_t> lags;
    EXPECT(noe_lag_check(nullptr, 0, 10, msg, sizeof msg) == -3 && strstr(msg, "K=0"), "K = 0: %s", msg);
    EXPECT(noe_lag_check(nullptr, -1, 10, msg, sizeof msg) == -3, "K = -1");
    lags.assign(kNoeMaxLags + 1, 0);
    for (size_t q = 0; q < lags.size(); ++q) lags[q] = (int32_t)q;
    EXPECT(noe_lag_check(lags.data(), kNoeMaxLags + 1, 1000, msg, sizeof msg) == -3 && strstr(msg, "K=65"), "K = 65: %s", msg);
    EXPECT(noe_lag_check(lags.data(), kNoeMaxLags, 1000, msg, sizeof msg) == 0, "K = 64");
    EXPECT(noe_lag_check(lags.data(), kNoeMaxLags, 64, msg, sizeof msg) == 0, "largest lag 63 in a block of 64");
    EXPECT(noe_lag_check(lags.data(), kNoeMaxLags, 63, msg, sizeof msg) == -3 && strstr(msg, "leaves no term"), "lag 63 in a block of 63: %s", msg);
    for (int K = 1; K <= 6; ++K)
        for (int bad = 0; bad < K; ++bad)
            for (int kind = 0; kind < 3; ++kind) {        // 0: a repeat, 1: a decrease, 2: a negative value
                lags.assign(K, 0);
                for (int q = 0; q < K; ++q) lags[q] = 3 * q + 1;
                if (kind == 0 && bad > 0) lags[bad] = lags[bad - 1];
                else if (kind == 1 && bad > 0) lags[bad] = lags[bad - 1] - 1;
                else if (kind == 2) lags[bad] = -1 - bad;
                const bool broken = kind == 2 || bad > 0;
                const int rc = noe_lag_check(lags.data(), K, 100, msg, sizeof msg);
                EXPECT(rc == (broken ? -3 : 0), "K %d bad %d kind %d: rc %d (%s)", K, bad, kind, rc, msg);
                if (broken) EXPECT(strstr(msg, kind == 2 ? "negative" : "strictly increasing"), "K %d bad %d kind %d: %s", K, bad, kind, msg);
            }
    lags = {0, INT32_MAX};
    EXPECT(noe_lag_check(lags.data(), 2, (int64_t)INT32_MAX + 1, msg, sizeof msg) == 0, "the largest lag");
    EXPECT(noe_lag_check(lags.data(), 2, INT32_MAX, msg, sizeof msg) == -3, "the largest lag in a block of its length");

    // ---- byte counts and grid sizes, against 128-bit restatements, up to the largest admitted shape ----
    for (int B : {1, 3, 65535, INT32_MAX})
        for (int K : {1, 12, 64})
            for (int64_t P : {(int64_t)2, (int64_t)33, (int64_t)512, (int64_t)40000, (int64_t)1 << 20})
                for (int S : {1, 2, 256}) {
                    const int64_t nT = (P + kNoeTile - 1) / kNoeTile, NP = nT * (nT + 1) / 2, npairs = P * (P - 1) / 2;
                    unsigned __int128 out, part;
                    noe_bytes(B, K, 1, npairs, S, NP, out, part);
                    unsigned __int128 want_out = 8, want_part = S > 1 ? 8 * 1024 : 0;
                    want_out *= (unsigned __int128)B; want_out *= (unsigned __int128)K; want_out *= (unsigned __int128)npairs;
                    want_part *= (unsigned __int128)B; want_part *= (unsigned __int128)K; want_part *= (unsigned __int128)S;
                    want_part *= (unsigned __int128)NP;
                    EXPECT(out == want_out && part == want_part, "bytes(B %d, K %d, P %lld, S %d)", B, K, (long long)P, S);
                    const unsigned __int128 wg = (unsigned __int128)B * K * S * NP, fin = (unsigned __int128)B * K * NP * 4;
                    const bool ok = wg < ((unsigned __int128)1 << 31) && fin < ((unsigned __int128)1 << 31);
                    EXPECT(noe_grid_ok(B, K, S, NP) == ok, "grid(B %d, K %d, P %lld, S %d)", B, K, (long long)P, S);
                    // the mode-resolved map: six sums per pair, the same grids
                    unsigned __int128 mout, mpart;
                    noe_bytes(B, K, kNoeModeSums, npairs, S, NP, mout, mpart);
                    EXPECT(mout == 6 * want_out && mpart == 6 * want_part, "modes bytes(B %d, K %d, P %lld, S %d)", B, K, (long long)P, S);
                    if (K > 1) continue;
                    // the map: one lag, seven sums per pair: 56 bytes per pair, 7 x 1024 float64 per partial tile
                    unsigned __int128 pout, ppart, want_pout = 56, want_ppart = S > 1 ? 7 * 8 * 1024 : 0;
                    want_pout *= (unsigned __int128)B; want_pout *= (unsigned __int128)npairs;
                    want_ppart *= (unsigned __int128)B; want_ppart *= (unsigned __int128)S; want_ppart *= (unsigned __int128)NP;
                    noe_bytes(B, 1, kNoeMapSums, npairs, S, NP, pout, ppart);
                    EXPECT(pout == want_pout && ppart == want_ppart, "map bytes(B %d, P %lld, S %d)", B, (long long)P, S);
                    const unsigned __int128 pwg = (unsigned __int128)B * S * NP, pfin = (unsigned __int128)B * NP * 4;
                    EXPECT(noe_grid_ok(B, 1, S, NP) == (pwg < ((unsigned __int128)1 << 31) && pfin < ((unsigned __int128)1 << 31)),
                           "map grid(B %d, P %lld, S %d)", B, (long long)P, S);
                }

    // ---- the frame matrix: the identity for NULL; orthogonal with determinant 1, R(q) v = q (0, v) q*, R(-q) = R(q), a scaling
    // inside the tolerance taken out; refusals ----
    {
        double Fm[9];
        EXPECT(noe_frame_matrix(nullptr, Fm, msg, sizeof msg) == 0, "NULL frame");
        for (int k = 0; k < 9; ++k) EXPECT(Fm[k] == (k % 4 == 0 ? 1.0 : 0.0), "identity[%d] = %g", k, Fm[k]);
        unsigned seed = 12345;
        auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (double)(seed >> 8) / (double)(1u << 24) - 0.5; };
        for (int n = 0; n < 2000; ++n) {
            double q[4] = {rnd(), rnd(), rnd(), rnd()};
            const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
            if (nq < 1e-3) continue;
            const double scale = 1.0 + 4e-7 * rnd();                // squared norm within 1e-6 of 1
            double qs[4], qn[4];
            for (int k = 0; k < 4; ++k) { q[k] /= nq; qs[k] = q[k] * scale; qn[k] = -q[k]; }
            double Fs[9], Fn[9];
            EXPECT(noe_frame_matrix(q, Fm, msg, sizeof msg) == 0 && noe_frame_matrix(qs, Fs, msg, sizeof msg) == 0 &&
                   noe_frame_matrix(qn, Fn, msg, sizeof msg) == 0, "unit quaternion %d refused: %s", n, msg);
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    double dot = 0.0;
                    for (int c = 0; c < 3; ++c) dot += Fm[3 * a + c] * Fm[3 * b + c];
                    EXPECT(std::fabs(dot - (a == b ? 1.0 : 0.0)) <= 1e-14, "rows %d, %d of frame %d: %g", a, b, n, dot);
                    EXPECT(std::fabs(Fs[3 * a + b] - Fm[3 * a + b]) <= 1e-14 && Fn[3 * a + b] == Fm[3 * a + b], "frame %d entry %d %d", n, a, b);
                }
            const double det = Fm[0] * (Fm[4] * Fm[8] - Fm[5] * Fm[7]) - Fm[1] * (Fm[3] * Fm[8] - Fm[5] * Fm[6]) + Fm[2] * (Fm[3] * Fm[7] - Fm[4] * Fm[6]);
            EXPECT(std::fabs(det - 1.0) <= 1e-14, "det of frame %d: %g", n, det);
            // q (0, v) q* by the quaternion product
            const double v[3] = {rnd(), rnd(), rnd()};
            const double w = q[0], x = q[1], y = q[2], z = q[3];
            const double tw = -x * v[0] - y * v[1] - z * v[2], tx = w * v[0] + y * v[2] - z * v[1], ty = w * v[1] + z * v[0] - x * v[2],
                         tz = w * v[2] + x * v[1] - y * v[0];
            const double rx = -tw * x + tx * w - ty * z + tz * y, ry = -tw * y + ty * w - tz * x + tx * z, rz = -tw * z + tz * w - tx * y + ty * x;
            for (int a = 0; a < 3; ++a) {
                const double got = Fm[3 * a] * v[0] + Fm[3 * a + 1] * v[1] + Fm[3 * a + 2] * v[2];
                EXPECT(std::fabs(got - (a == 0 ? rx : a == 1 ? ry : rz)) <= 1e-14, "frame %d rotates component %d to %g", n, a, got);
            }
        }
        const double bad[][4] = {{1.0, 0.1, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {1.0 + 1e-6, 0.0, 0.0, 0.0}, {0.999999, 0.0, 0.0, 0.0}};
        for (const auto &qb : bad) EXPECT(noe_frame_matrix(qb, Fm, msg, sizeof msg) == -3 && strstr(msg, "not a unit quaternion"), "norm: %s", msg);
        for (int k = 0; k < 4; ++k)
            for (double v : {(double)NAN, (double)INFINITY, -(double)INFINITY}) {
                double qb[4] = {1.0, 0.0, 0.0, 0.0};
                qb[k] = v;
                EXPECT(noe_frame_matrix(qb, Fm, msg, sizeof msg) == -3 && strstr(msg, "is not finite"), "component %d = %g: %s", k, v, msg);
            }
    }
    printf("noe_lagged_host_sweep: %ld comparisons, no disagreement\n", checks);
    return 0;
}
