// sr_pack_tile.h -- the register tile of kernel 0, shared by k_pack_soa (sr_pack.hip) and the C(t) kernel that carries the next
// batch's pack (k_ct_rfft32 with PACK set, sr_ct32.hip).
//
// One 256-thread workgroup moves a tile of 128 frames x 32 vectors from the frame-major array (N, Vtot, 3) to the planes
// soa[(v*3+c)*Npad + n].  A thread owns three 4 x 4 blocks -- four consecutive frames x one 16-byte column of a frame's row (four
// consecutive components) -- twelve 16-byte loads all in flight, then twelve 16-byte stores; the lanes of a wave are 8 columns x 8
// frame groups, so a wave-load reads 8 full 128-byte lines (8 frames) and a wave-store writes 8 full lines (128 B of each of 8
// planes).  Both sides non-temporal: the vectors are read once, the planes are next read by another kernel (or another launch).
// Requires whole 32-vector tiles and 16-byte aligned rows: nV % 32 == 0, (Vtot * 3) % 4 == 0, (v0 * 3) % 4 == 0, vecs and soa
// 16-byte aligned, Npad % 4 == 0 (sr_pack_reg_tiles / the callers check).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int kPackVecs = 32;           // vectors per tile (both forms of the pack)
constexpr int kPackRegFrames = 128;     // frames per register tile

typedef float sr_v4f __attribute__((ext_vector_type(4)));

// the loads of tile (tile_x, tile_y): frames [128 tile_x, +128), vectors [32 tile_y, +32) of the shard that starts at v0.
// No branch around a load: past the end, frame N - 1 again.  IT0, IT1: the thread's blocks [IT0, IT1) of its three only (a caller
// short of registers moves a tile in parts).
template <int IT0 = 0, int IT1 = 3>
__device__ __forceinline__ void sr_pack_tile_load(sr_v4f (&r)[3][4], const float *__restrict__ vecs, int64_t N, int64_t Vtot, int64_t v0,
                                                  int64_t tile_x, int64_t tile_y)
{
    const int64_t n0 = tile_x * kPackRegFrames, vb = tile_y * kPackVecs;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ql = lane & 7, gl = lane >> 3;
#pragma unroll
    for (int it = IT0; it < IT1; ++it) {
        const int blk = it * 4 + wave;                        // 12 wave-blocks: 3 column groups x 4 groups of 8 frame groups
        const int q = (blk % 3) * 8 + ql;                     // 16-byte column of the 96-float row
        const int64_t fr = n0 + 4 * ((blk / 3) * 8 + gl);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t f = min(fr + j, N - 1);
            r[it][j] = __builtin_nontemporal_load(reinterpret_cast<const sr_v4f *>(vecs + (f * Vtot + v0 + vb) * 3 + 4 * q));
        }
    }
}

// the stores of the same tile: zeros for frames in [N, Npad), nothing at or beyond Npad
template <int IT0 = 0, int IT1 = 3>
__device__ __forceinline__ void sr_pack_tile_store(sr_v4f (&r)[3][4], int64_t N, float *__restrict__ soa, int64_t Npad, int64_t tile_x,
                                                   int64_t tile_y)
{
    const int64_t n0 = tile_x * kPackRegFrames, vb = tile_y * kPackVecs;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ql = lane & 7, gl = lane >> 3;
#pragma unroll
    for (int it = IT0; it < IT1; ++it) {
        const int blk = it * 4 + wave;
        const int q = (blk % 3) * 8 + ql;
        const int64_t fr = n0 + 4 * ((blk / 3) * 8 + gl);
        if (fr >= Npad) continue;                             // Npad % 4 == 0: a frame group is inside the planes or outside
        if (fr + 3 >= N) {                                    // frames in [N, Npad): zeros
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (fr + j >= N) r[it][j] = sr_v4f{0.f, 0.f, 0.f, 0.f};
        }
        float *o = soa + (vb * 3 + 4 * q) * Npad + fr;
        __builtin_nontemporal_store(sr_v4f{r[it][0].x, r[it][1].x, r[it][2].x, r[it][3].x}, reinterpret_cast<sr_v4f *>(o));
        __builtin_nontemporal_store(sr_v4f{r[it][0].y, r[it][1].y, r[it][2].y, r[it][3].y}, reinterpret_cast<sr_v4f *>(o + Npad));
        __builtin_nontemporal_store(sr_v4f{r[it][0].z, r[it][1].z, r[it][2].z, r[it][3].z}, reinterpret_cast<sr_v4f *>(o + 2 * Npad));
        __builtin_nontemporal_store(sr_v4f{r[it][0].w, r[it][1].w, r[it][2].w, r[it][3].w}, reinterpret_cast<sr_v4f *>(o + 3 * Npad));
    }
}

__device__ __forceinline__ void sr_pack_tile(const float *__restrict__ vecs, int64_t N, int64_t Vtot, int64_t v0, float *__restrict__ soa,
                                             int64_t Npad, int64_t tile_x, int64_t tile_y)
{
    sr_v4f r[3][4];
    sr_pack_tile_load(r, vecs, N, Vtot, v0, tile_x, tile_y);
    sr_pack_tile_store(r, N, soa, Npad, tile_x, tile_y);
}

// A pack job carried by another kernel's launch: its workgroups take tiles b, b + gridDim.x, ... in k_pack_soa's block order
// (tile = tile_y * tiles_x + tile_x).  tiles == 0: no job.
struct sr_pack_job {
    const float *vecs;
    float *soa;
    int64_t N, Vtot, v0, Npad;
    int tiles_x, tiles;
};
