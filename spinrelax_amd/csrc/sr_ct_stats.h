// sr_ct_stats.h -- the chunk statistics of one (series row, lag): what k_ct_finalize (sr_ct.hip) computes per thread, for kernels that
// take C(t) and dC(t) straight from kernel 1's raw sums (k_order_search with a raw-sum source, sr_fit.hip).
//
// calculate-Ct-from-traj.py:226-228: C_r = 1.5 S_r / n - 0.5 per chunk, m = mean over the chunks in chunk order, the deviation in two
// passes (numpy.std) and sd = sqrt(s / R) / (sqrt(R) - 1).  R = 1 gives 0 / 0 like the reference.
//
// Rounding.  k_ct_finalize is compiled with floating-point contraction on, and the compiler fuses there what can be fused:
// 1.5 q - 0.5 is ONE fma, and so is every s + e e of the deviation.  The same operations are written out here -- fma() where
// k_ct_finalize's code has a fused one, plain operations under contract(off) everywhere else -- so that this function gives its bits
// whatever the including file is compiled with (tests/test_gpu_fused_stats.py compares the two on integer views, with inputs whose
// 1.5 q - 0.5 differs in the last bit between the fused and the unfused form).
#pragma once

constexpr int kStatsR = 32;        // replicate chunks kept in registers (k_ct_finalize's kFinR); more: two passes over memory

// p: the raw sum of chunk 0 at this lag; chunk r is at p[r * Lp].  n = F - lag, rootR = sqrt((double)R) - 1.0.
__device__ __forceinline__ void sr_ct_chunk_stats(const double *__restrict__ p, int64_t Lp, int R, double n, double rootR, double &m_out,
                                                  double &sd_out)
{
#pragma clang fp contract(off)
    double m = 0.0, s = 0.0;
    if (R <= kStatsR) {
        // every load of the point in flight before the first use
        double pr[kStatsR];
#pragma unroll
        for (int r = 0; r < kStatsR; ++r) pr[r] = r < R ? p[(int64_t)r * Lp] : 0.0;
#pragma unroll
        for (int r = 0; r < kStatsR; ++r) {
            pr[r] = fma(1.5, pr[r] / n, -0.5);
            if (r < R) m += pr[r];
        }
        m /= (double)R;
#pragma unroll
        for (int r = 0; r < kStatsR; ++r) {
            const double e = pr[r] - m;
            if (r < R) s = fma(e, e, s);
        }
    } else {
        for (int r = 0; r < R; ++r) m += fma(1.5, p[(int64_t)r * Lp] / n, -0.5);
        m /= (double)R;
        for (int r = 0; r < R; ++r) {
            const double e = fma(1.5, p[(int64_t)r * Lp] / n, -0.5) - m;
            s = fma(e, e, s);
        }
    }
    m_out = m;
    sd_out = sqrt(s / (double)R) / rootR;
}
