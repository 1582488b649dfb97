// sr_pack_planes.h -- the tile transpose of the plane packs that feed the staged correlation kernels: k_pack_dipolar
// (sr_ct_dipolar.hip: four planes per vector) and k_pack_modes (sr_ct_modes.hip: five).  Frame-major vectors vecs[(f * Vtot + v) * 3]
// become NPL planes per vector in kernel 0's layout, soa[(v * NPL + c) * Npad + n], zero for n in [N, Npad).  One workgroup of 256
// threads takes 64 frames of 32 vectors: it reads frame by frame (a frame's 32 vectors are 96 consecutive floats), computes the NPL
// values of every (frame, vector) with the caller's function, and writes plane by plane through an LDS tile, 64 consecutive frames per
// row.  Kernel 0's own pack (k_pack_soa, sr_pack_tile.h) is another tile: three planes, no arithmetic, carried inside k_ct_rfft32.
#pragma once
#include "sr_internal.h"

namespace {

constexpr int kPlaneVecs = 32;          // vectors per tile
constexpr int kPlaneFrames = 64;        // frames per tile

// frame(p, di, v, o): p the three floats of one vector in one frame, di its index in the frame-major array (f * Vtot + v0 + v), v the
// vector's number in this call; fills o[0 .. NPL) (zero on entry).  Launch: 256 threads, grid of pack_planes_grid
template <int NPL, class Frame>
__device__ __forceinline__ void pack_planes_tile(const float *__restrict__ vecs, int64_t N, int64_t Vtot, int64_t v0, int64_t nV,
                                                 float *__restrict__ soa, int64_t Npad, Frame frame)
{
    __shared__ float tile[kPlaneVecs * NPL][kPlaneFrames + 1];
    const int64_t n0 = (int64_t)blockIdx.x * kPlaneFrames;
    const int64_t vb = (int64_t)blockIdx.y * kPlaneVecs;
    const int nvec = (int)min((int64_t)kPlaneVecs, nV - vb);
    const int tid = threadIdx.x;
    for (int idx = tid; idx < kPlaneFrames * nvec; idx += 256) {
        const int n = idx / nvec, k = idx - n * nvec;
        const int64_t fr = n0 + n;
        float o[NPL];
#pragma unroll
        for (int c = 0; c < NPL; ++c) o[c] = 0.f;
        if (fr < N) frame(vecs + (fr * Vtot + v0 + vb + k) * 3, fr * Vtot + v0 + vb + k, vb + k, o);
#pragma unroll
        for (int c = 0; c < NPL; ++c) tile[k * NPL + c][n] = o[c];
    }
    __syncthreads();
    const int row = nvec * NPL;
    for (int idx = tid; idx < kPlaneFrames * row; idx += 256) {
        const int k = idx / kPlaneFrames, n = idx - k * kPlaneFrames;
        const int64_t fr = n0 + n;
        if (fr < Npad) soa[(vb * NPL + k) * Npad + fr] = tile[k][n];
    }
}

// what both packs refuse (-3) before anything is queued, and their grid: x the tiles of frames, y the tiles of vectors
inline int pack_planes_grid(const char *who, int64_t N, int64_t Vtot, int64_t v0, int64_t nV, int64_t Npad, dim3 &grid)
{
    SR_REQUIRE(N > 0 && Vtot > 0 && nV > 0 && v0 >= 0 && v0 + nV <= Vtot, -3, "%s: bad shape N=%lld Vtot=%lld v0=%lld nV=%lld", who, (long long)N,
               (long long)Vtot, (long long)v0, (long long)nV);
    SR_REQUIRE(Npad >= N && Npad % 4 == 0, -3, "%s: Npad=%lld must be >= N and a multiple of 4", who, (long long)Npad);
    const int64_t gx = (Npad + kPlaneFrames - 1) / kPlaneFrames;
    const int64_t gy = (nV + kPlaneVecs - 1) / kPlaneVecs;
    SR_REQUIRE(gy <= 65535, -3, "%s: too many vectors in one call (%lld)", who, (long long)nV);
    grid = dim3((unsigned)gx, (unsigned)gy);
    return 0;
}

}  // namespace
