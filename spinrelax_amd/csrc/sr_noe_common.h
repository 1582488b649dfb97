// sr_noe_common.h -- what the all-pairs dipolar map (sr_noe.hip) and its lagged form (sr_noe_lagged.hip) share: the tile order, the
// arithmetic helpers of the two precisions, the checked shape
#pragma once
#include "sr_internal.h"
#include "sr_noe_host.h"

#ifdef __HIPCC__
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
#endif

struct NoeShape {
    int64_t nT, NP, npairs, Fmax;
    int S;
};

// everything that the map refuses, before anything is queued (sr_noe.hip); fills sh
int noe_check(sr_ctx *ctx, const char *who, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const int64_t *bs,
              const int64_t *bl, int B, int mode, NoeShape &sh);
