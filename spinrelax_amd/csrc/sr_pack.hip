// sr_pack.hip -- kernel 0 for gfx950: frame-major bond vectors (N, Vtot, 3) float32 -> per-vector planes, the layout every
// form of kernel 1 (sr_ct.hip) and the histogram kernels read.  Three kernels: whole 32-vector tiles in registers (production),
// any shape through an LDS tile, and the LDS tile with the per-frame de-tumbling rotation folded in.
#include "sr_internal.h"
#include "sr_pack_tile.h"

namespace {

// ------------------------------------------------------------------------------------------
// kernel 0: (N, Vtot, 3) float32 -> planes soa[(v*3+c)*Npad + n], zero for n in [N, Npad)
// ------------------------------------------------------------------------------------------
constexpr int kPackFrames = 64;          // (kPackVecs = 32, kPackRegFrames = 128: sr_pack_tile.h)

// The general form (any number of vectors, any alignment): a 64-frame x 32-vector tile transposed through LDS.
// 16-byte accesses on both sides when it can: a frame's 32 vectors are 96 consecutive floats (24 float4 when the row start is
// 16-byte aligned, i.e. Vtot*3 and (v0+vb)*3 multiples of 4), a plane row of 64 frames is 16 float4.
__global__ __launch_bounds__(256) void k_pack_soa_ragged(const float *__restrict__ vecs, int64_t N, int64_t Vtot,
                                                         int64_t v0, int64_t nV, float *__restrict__ soa, int64_t Npad)
{
    __shared__ float tile[kPackVecs * 3][kPackFrames + 1];
    const int64_t n0 = (int64_t)blockIdx.x * kPackFrames;
    const int64_t vb = (int64_t)blockIdx.y * kPackVecs;
    const int nvec = (int)min((int64_t)kPackVecs, nV - vb);
    const int row = nvec * 3;
    const int tid = threadIdx.x;
    const bool vec4 = ((Vtot * 3) & 3) == 0 && (((v0 + vb) * 3) & 3) == 0 && (row & 3) == 0;
    if (vec4) {
        const int q4 = row >> 2;                              // float4 per frame
        for (int idx = tid; idx < kPackFrames * q4; idx += 256) {
            const int n = idx / q4, q = idx - n * q4;
            const int64_t fr = n0 + n;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (fr < N) val = *reinterpret_cast<const float4 *>(vecs + (fr * Vtot + v0 + vb) * 3 + 4 * q);
            tile[4 * q + 0][n] = val.x;
            tile[4 * q + 1][n] = val.y;
            tile[4 * q + 2][n] = val.z;
            tile[4 * q + 3][n] = val.w;
        }
    } else {
        for (int idx = tid; idx < kPackFrames * row; idx += 256) {
            const int n = idx / row, k = idx - n * row;
            const int64_t fr = n0 + n;
            float val = 0.f;
            if (fr < N) val = vecs[(fr * Vtot + v0 + vb) * 3 + k];
            tile[k][n] = val;
        }
    }
    __syncthreads();
    // Npad % 4 == 0 and n0 % 64 == 0: every group of four frames is either fully inside the planes or fully outside
    for (int idx = tid; idx < (kPackFrames / 4) * row; idx += 256) {
        const int k = idx / (kPackFrames / 4), n = (idx - k * (kPackFrames / 4)) * 4;
        const int64_t fr = n0 + n;
        if (fr < Npad) {
            const float4 o = make_float4(tile[k][n], tile[k][n + 1], tile[k][n + 2], tile[k][n + 3]);
            *reinterpret_cast<float4 *>(soa + (vb * 3 + k) * Npad + fr) = o;
        }
    }
}

// The production form (whole 32-vector tiles, 16-byte aligned rows: cfg3 / cfg4 and every shard of them): the transposition in
// REGISTERS, no LDS.  A thread owns three 4 x 4 blocks -- four consecutive frames x one 16-byte column of a frame's row (four
// consecutive components) -- twelve 16-byte loads all in flight, then twelve 16-byte stores; the lanes of a wave are 8 columns x 8
// frame groups, so a wave-load reads 8 full 128-byte lines (8 frames) and a wave-store writes 8 full lines (128 B of each of 8
// planes).  Both sides non-temporal: the vectors are read once, the planes are next read by another kernel.  Measured against the
// LDS tile above (round 4, scripts/dev/interference.py, same box each time): alone 0.208-0.223 against 0.229-0.239 ms (5.5-5.9
// TB/s), and what one pack costs 20 back-to-back C(t) launches it runs beside 0.165-0.185 against 0.197-0.207 ms; 20-step
// benchmark 2.27-2.32 against 2.35-2.38 ms per step.  The LDS tile's scattered 4-byte LDS writes and its 54 instructions per 16
// bytes were what the C(t) waves on the same CU paid for.  (An LDS-DMA fill of the same tile: no gain; 16 or 4 columns per wave,
// temporal accesses, four loads in flight instead of twelve: worse or equal.)
__global__ __launch_bounds__(256) void k_pack_soa(const float *__restrict__ vecs, int64_t N, int64_t Vtot,
                                                  int64_t v0, int64_t nV, float *__restrict__ soa, int64_t Npad)
{
    sr_pack_tile(vecs, N, Vtot, v0, soa, Npad, blockIdx.x, blockIdx.y);      // sr_pack_tile.h: shared with k_ct_rfft32's carried pack
}

// The same transposition with the de-tumbling folded in: every frame's vectors are rotated by that frame's unit
// quaternion (float64, rotate_vector_simd's operation order, transforms3d_supplement.py:270-296) and rounded to the
// float32 the planes hold.  SURVEY.md section 8(f)-1: lab-frame vectors + colvar-qorient in, body-frame C(t) out.
__global__ __launch_bounds__(256) void k_pack_soa_rot(const float *__restrict__ vecs, int64_t N, int64_t Vtot, int64_t v0,
                                                      int64_t nV, const double *__restrict__ quat,
                                                      float *__restrict__ soa, int64_t Npad)
{
#pragma clang fp contract(off)
    __shared__ float tile[kPackVecs * 3][kPackFrames + 1];
    const int64_t n0 = (int64_t)blockIdx.x * kPackFrames;
    const int64_t vb = (int64_t)blockIdx.y * kPackVecs;
    const int nvec = (int)min((int64_t)kPackVecs, nV - vb);
    const int tid = threadIdx.x;
    for (int idx = tid; idx < kPackFrames * nvec; idx += 256) {
        const int n = idx / nvec, k = idx - n * nvec;
        const int64_t fr = n0 + n;
        float ox = 0.f, oy = 0.f, oz = 0.f;
        if (fr < N) {
            const float *p = vecs + (fr * Vtot + v0 + vb + k) * 3;
            const double vx = (double)p[0], vy = (double)p[1], vz = (double)p[2];
            const double qw = quat[fr * 4 + 0], qx = quat[fr * 4 + 1], qy = quat[fr * 4 + 2], qz = quat[fr * 4 + 3];
            const double ax = (qy * vz - qz * vy) + qw * vx;
            const double ay = (qz * vx - qx * vz) + qw * vy;
            const double az = (qx * vy - qy * vx) + qw * vz;
            const double bx = qy * az - qz * ay;
            const double by = qz * ax - qx * az;
            const double bz = qx * ay - qy * ax;
            ox = (float)((bx + bx) + vx);
            oy = (float)((by + by) + vy);
            oz = (float)((bz + bz) + vz);
        }
        tile[k * 3 + 0][n] = ox;
        tile[k * 3 + 1][n] = oy;
        tile[k * 3 + 2][n] = oz;
    }
    __syncthreads();
    const int row = nvec * 3;
    for (int idx = tid; idx < kPackFrames * row; idx += 256) {
        const int k = idx / kPackFrames, n = idx - k * kPackFrames;
        const int64_t fr = n0 + n;
        if (fr < Npad) soa[(vb * 3 + k) * Npad + fr] = tile[k][n];
    }
}

}  // namespace

// what sr_pack_soa_f32_dev refuses, before anything is queued (shared with sr_ct_palmer_sums_pack_f32_dev, sr_ct.hip)
int sr_pack_soa_check(const char *who, const float *vecs, int64_t N, int64_t Vtot, int64_t v0, int64_t nV, const float *soa, int64_t Npad)
{
    SR_REQUIRE(vecs && soa, -2, "%s: null pointer", who);
    SR_REQUIRE(N > 0 && Vtot > 0 && nV > 0 && v0 >= 0 && v0 + nV <= Vtot, -3, "%s: bad shape N=%lld Vtot=%lld v0=%lld nV=%lld", who,
               (long long)N, (long long)Vtot, (long long)v0, (long long)nV);
    SR_REQUIRE(Npad >= N && Npad % 4 == 0, -3, "%s: Npad=%lld must be >= N and a multiple of 4", who, (long long)Npad);
    SR_REQUIRE((nV + kPackVecs - 1) / kPackVecs <= 65535, -3, "%s: too many vectors in one call (%lld)", who, (long long)nV);
    return 0;
}

extern "C" {

int64_t sr_pack_reg_tiles(int64_t Npad, int64_t Vtot, int64_t v0, int64_t nV)
{
    if (Npad < 4 || (Npad & 3) || Vtot < 1 || v0 < 0 || nV < 1 || v0 + nV > Vtot) return 0;
    if (nV % kPackVecs != 0 || ((Vtot * 3) & 3) != 0 || ((v0 * 3) & 3) != 0) return 0;
    return ((Npad + kPackRegFrames - 1) / kPackRegFrames) * (nV / kPackVecs);
}

int sr_pack_soa_f32_dev(sr_ctx *ctx, const float *vecs, int64_t N, int64_t Vtot, int64_t v0, int64_t nV,
                        float *soa, int64_t Npad)
{
    SR_CHECK_CTX(ctx);
    if (int rc = sr_pack_soa_check("sr_pack_soa_f32_dev", vecs, N, Vtot, v0, nV, soa, Npad)) return rc;
    const int64_t gx = (Npad + kPackFrames - 1) / kPackFrames;
    const int64_t gy = (nV + kPackVecs - 1) / kPackVecs;
    if (sr_pack_reg_tiles(Npad, Vtot, v0, nV) > 0 && (((uintptr_t)vecs | (uintptr_t)soa) & 15) == 0)
        hipLaunchKernelGGL(k_pack_soa, dim3((unsigned)((Npad + kPackRegFrames - 1) / kPackRegFrames), (unsigned)gy), dim3(256), 0,
                           ctx->stream, vecs, N, Vtot, v0, nV, soa, Npad);
    else
        hipLaunchKernelGGL(k_pack_soa_ragged, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, ctx->stream, vecs, N, Vtot, v0, nV,
                           soa, Npad);
    SR_HIP(hipGetLastError());
    return 0;
}

int sr_pack_soa_rot_f32_dev(sr_ctx *ctx, const float *vecs, int64_t N, int64_t Vtot, int64_t v0, int64_t nV,
                            const double *quat, float *soa, int64_t Npad)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(vecs && soa && quat, -2, "sr_pack_soa_rot_f32_dev: null pointer");
    SR_REQUIRE(N > 0 && Vtot > 0 && nV > 0 && v0 >= 0 && v0 + nV <= Vtot, -3,
               "sr_pack_soa_rot_f32_dev: bad shape N=%lld Vtot=%lld v0=%lld nV=%lld", (long long)N, (long long)Vtot,
               (long long)v0, (long long)nV);
    SR_REQUIRE(Npad >= N && Npad % 4 == 0, -3, "sr_pack_soa_rot_f32_dev: Npad=%lld must be >= N and a multiple of 4",
               (long long)Npad);
    const int64_t gx = (Npad + kPackFrames - 1) / kPackFrames;
    const int64_t gy = (nV + kPackVecs - 1) / kPackVecs;
    SR_REQUIRE(gy <= 65535, -3, "sr_pack_soa_rot_f32_dev: too many vectors in one call (%lld)", (long long)nV);
    hipLaunchKernelGGL(k_pack_soa_rot, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, ctx->stream, vecs, N, Vtot, v0, nV,
                       quat, soa, Npad);
    SR_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
