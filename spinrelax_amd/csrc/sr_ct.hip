// sr_ct.hip -- kernel 1 (Palmer-chunked P2 autocorrelation) for gfx950: which formulation runs for a chunk length, the reduction
// over the replicate chunks that all of them share (k_ct_finalize), and the entry points.
//
// Reference semantics: calculate_Ct_Palmer, calculate-Ct-from-traj.py:200-238 (see include/spinrelax_hip.h).
//
// Every formulation produces the same raw sums S[lag] = sum_j (u(j).u(j+lag))^2, lag = 1 .. L = F/2, per (vector, chunk) series
// in psum (nV, R, Lp); k_ct_finalize turns them into C(t) and dC(t).  Five of them, one file and one launcher each:
//   SR_CT_DIRECT   sr_ct_direct.hip  k_ct_palmer   shifted products, float32 dot products (mode 1: float64 throughout); the series
//                                                  is staged in LDS, 12 bytes per frame: F up to about 13400
//   SR_CT_FFT64    sr_ct_fft64.hip   k_ct_fft      Wiener-Khinchin, complex float64 transforms of 2048 .. 8192 points in LDS (1e-15)
//   SR_CT_RFFT64   sr_ct_fft64.hip   k_ct_rfft     the same with real-input transforms of half the length, 6144 and 8192 points
//   SR_CT_RFFT32   sr_ct32.hip       k_ct_rfft32   float32 real-input transforms of the mean-removed traceless components (6e-8 on
//                                                  ordered, 1.6e-7 on mobile vectors: the class of the direct kernel): the pipeline's
//   SR_CT_BLOCKED  sr_ct_long.hip    k_ctl_*       blocked float32 transforms through device memory: F up to 262144
// Kernel 0, which packs the planes they all read, is sr_pack.hip.
//
// The rule (sr_ct_formulation; need = F + L is what one transform must hold, "fits" = the direct kernel can stage the chunk):
//   mode 1                                                         direct if it fits, else refused
//   mode 0, ct_fft >= 2, need > 8192, F >= ct_long_min_frames      blocked
//   mode 0, ct_fft >= 2, need > 8192, does not fit                 blocked
//   anything else that does not fit                                refused (-4)
//   ct_fft = 0, or need <= 1024 (cheap anyway), or need > 8192     direct
//   ct_fft = 4, or ct_fft = 3 with need > 4096                     float32 transforms     (N1 = 4, 8, 12, 16 by need <= 2048 .. 8192)
//   ct_fft = 2 with need > 4096                                    real float64           (N1 = 12 for need <= 6144, else 16)
//   otherwise (ct_fft = 1; 2 and 3 with need <= 4096)              complex float64        (N1 = 8, 16, 24, 32 by need <= 2048 .. 8192)
// ct_fft defaults to 3: cfg3 / cfg4 (F = 4096) run float32 transforms, cfg2's shorter chunks complex float64 ones (why: the note
// above sr_launch_ct_rfft32).  ct_long_min_frames defaults to SR_CT_LONG_MIN_FRAMES = 16384, above what fits: by default the
// blocked form takes exactly the chunks the direct kernel cannot stage, and the option hands it shorter ones (from 5462 frames).
#include "sr_internal.h"
#include "sr_ct_shift.h"        // ct_Fp, kPad: the frames a staged series takes
#include "sr_pack_tile.h"

namespace {

// mean / std over the R replicate chunks, calculate-Ct-from-traj.py:226-228.  One workgroup owns a tile of kFinV vectors x
// kFinD lags: the raw sums are read along the lags (a wave = 64 consecutive lags of one vector), the results leave in BOTH
// orientations -- (lags, vectors) as the reference holds them, through an LDS tile so that 16 consecutive vectors of a lag
// go out together, and (vectors, lags) for the fit, straight from the registers.  (The thread-per-element version wrote
// the (lags, vectors) arrays with a stride of nV doubles: 445 MB of HBM traffic for 218 MB of data, and two transposition
// launches behind it.)
constexpr int kFinV = 16, kFinD = 64;
constexpr int kFinR = 32;          // replicate chunks a thread keeps in registers (more: two passes over memory)
// half: what is subtracted from 1.5 S / n per chunk -- 0.5 for unit vectors (P2 = 1.5 cos^2 - 0.5); 0 for the distance-weighted
// functions, whose raw sums S_a - S_w / 3 carry the whole function (sr_ct_dipolar.hip)
__global__ __launch_bounds__(256) void k_ct_finalize(const double *__restrict__ psum, int R, int F, int L, int Lp,
                                                     int64_t nV, double half, double *__restrict__ Ct, double *__restrict__ dCt,
                                                     double *__restrict__ CtT, double *__restrict__ dCtT)
{
    __shared__ double tm[kFinV][kFinD + 1], ts[kFinV][kFinD + 1];
    const int tid = threadIdx.x;
    const int d0 = blockIdx.x * kFinD;                  // lag index - 1 of the tile's first column
    const int64_t v0 = (int64_t)blockIdx.y * kFinV;
    const double rootR = sqrt((double)R) - 1.0;
    {
        const int dl = tid & 63;
        const int d = d0 + dl + 1;
#pragma unroll
        for (int i = 0; i < kFinV / 4; ++i) {
            const int vl = (tid >> 6) + 4 * i;
            const int64_t v = v0 + vl;
            if (d > L || v >= nV) continue;
            const double *p = psum + v * R * Lp + d;
            const double n = (double)(F - d);
            double m = 0.0, s = 0.0;
            if (R <= kFinR) {
                // the replicate values stay in registers between the two passes of numpy.std: the raw sums (201 MB for cfg3)
                // are read once, all loads in flight together
                double pr[kFinR];
#pragma unroll
                for (int r = 0; r < kFinR; ++r) pr[r] = r < R ? p[(int64_t)r * Lp] : 0.0;
#pragma unroll
                for (int r = 0; r < kFinR; ++r) {
                    pr[r] = 1.5 * (pr[r] / n) - half;
                    if (r < R) m += pr[r];
                }
                m /= (double)R;
#pragma unroll
                for (int r = 0; r < kFinR; ++r) {
                    const double e = pr[r] - m;
                    if (r < R) s += e * e;
                }
            } else {
                for (int r = 0; r < R; ++r) m += 1.5 * (p[(int64_t)r * Lp] / n) - half;
                m /= (double)R;
                for (int r = 0; r < R; ++r) {
                    const double e = (1.5 * (p[(int64_t)r * Lp] / n) - half) - m;
                    s += e * e;
                }
            }
            const double sd = sqrt(s / (double)R) / rootR;
            tm[vl][dl] = m;
            ts[vl][dl] = sd;
            if (CtT) {
                CtT[v * L + (d - 1)] = m;
                dCtT[v * L + (d - 1)] = sd;
            }
        }
    }
    __syncthreads();
    {
        const int vl = tid & 15;
        const int64_t v = v0 + vl;
#pragma unroll
        for (int i = 0; i < kFinD / 16; ++i) {
            const int dl = (tid >> 4) + 16 * i;
            const int d = d0 + dl + 1;
            if (d > L || v >= nV) continue;
            const int64_t o = (int64_t)(d - 1) * nV + v;
            Ct[o] = tm[vl][dl];
            dCt[o] = ts[vl][dl];
        }
    }
}

__global__ __launch_bounds__(256) void k_transpose_f64(const double *__restrict__ in, int64_t rows, int64_t cols,
                                                       double *__restrict__ out)
{
    __shared__ double tile[32][33];
    const int64_t c0 = (int64_t)blockIdx.x * 32, r0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8)
        if (r0 + k < rows && c0 + tx < cols) tile[k][tx] = in[(r0 + k) * cols + c0 + tx];
    __syncthreads();
    for (int k = ty; k < 32; k += 8)
        if (c0 + k < cols && r0 + tx < rows) out[(c0 + k) * rows + r0 + tx] = tile[tx][k];
}

// g matrices (rows, cols), one behind the other, each to (cols, rows): the tile of k_transpose_f64 with the matrix on grid.z
__global__ __launch_bounds__(256) void k_transpose_batched_f64(const double *__restrict__ in, int64_t rows, int64_t cols,
                                                               double *__restrict__ out)
{
    __shared__ double tile[32][33];
    const int64_t c0 = (int64_t)blockIdx.x * 32, r0 = (int64_t)blockIdx.y * 32;
    const int64_t base = (int64_t)blockIdx.z * rows * cols;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8)
        if (r0 + k < rows && c0 + tx < cols) tile[k][tx] = in[base + (r0 + k) * cols + c0 + tx];
    __syncthreads();
    for (int k = ty; k < 32; k += 8)
        if (c0 + k < cols && r0 + tx < rows) out[base + (c0 + k) * rows + r0 + tx] = tile[tx][k];
}

}  // namespace

extern "C" {

int sr_transpose_batched_f64_dev(sr_ctx *ctx, const double *in, int64_t g, int64_t rows, int64_t cols, double *out)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(in && out, -2, "sr_transpose_batched_f64_dev: null pointer");
    SR_REQUIRE(g > 0 && rows > 0 && cols > 0, -3, "sr_transpose_batched_f64_dev: bad shape g=%lld rows=%lld cols=%lld", (long long)g,
               (long long)rows, (long long)cols);
    const int64_t gx = (cols + 31) / 32, gy = (rows + 31) / 32;
    SR_REQUIRE(gy <= 65535 && g <= 65535 && gx < ((int64_t)1 << 31), -3, "sr_transpose_batched_f64_dev: too many rows or matrices");
    hipLaunchKernelGGL(k_transpose_batched_f64, dim3((unsigned)gx, (unsigned)gy, (unsigned)g), dim3(256), 0, ctx->stream, in, rows, cols,
                       out);
    SR_HIP(hipGetLastError());
    return 0;
}

int sr_transpose_f64_dev(sr_ctx *ctx, const double *in, int64_t rows, int64_t cols, double *out)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(in && out && rows > 0 && cols > 0, -2, "sr_transpose_f64_dev: bad arguments");
    const int64_t gx = (cols + 31) / 32, gy = (rows + 31) / 32;
    SR_REQUIRE(gy <= 65535, -3, "sr_transpose_f64_dev: too many rows");
    hipLaunchKernelGGL(k_transpose_f64, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, ctx->stream, in, rows, cols, out);
    SR_HIP(hipGetLastError());
    return 0;
}

int64_t sr_ct_psum_stride(int64_t F) { return sr_round_up(F / 2 + 1 + kLagBlock, 8); }

int64_t sr_ct_max_frames_per_chunk(sr_ctx *ctx)
{
    if (!ctx) return -1;
    return SR_CT_LONG_MAX_FRAMES;        // the blocked transforms of the default dispatch (sr_ct_long.hip)
}

int sr_ct_formulation(int ct_fft, int64_t ct_long_min_frames, int mode, int64_t F, int64_t lds_limit)
{
    if (ct_fft < 0 || ct_fft > 4 || (mode != 0 && mode != 1) || F < 2 || F > SR_CT_LONG_MAX_FRAMES) return SR_CT_REFUSED;
    const int64_t need = F + F / 2;
    const bool fits_direct = (int64_t)sr_ct_direct_lds_bytes(F) <= lds_limit;
    if (mode == 0 && ct_fft >= 2 && need > 8192 && (F >= ct_long_min_frames || !fits_direct)) return SR_CT_BLOCKED;
    if (!fits_direct) return SR_CT_REFUSED;
    if (mode == 1 || ct_fft == 0 || need <= 1024 || need > 8192) return SR_CT_DIRECT;
    if (ct_fft == 4 || (ct_fft == 3 && need > 4096)) return SR_CT_RFFT32;
    if (ct_fft == 2 && need > 4096) return SR_CT_RFFT64;
    return SR_CT_FFT64;
}

int sr_ct_pack_fused(int formulation, int64_t F, int64_t series, int64_t tiles, int aligned)
{
    // k_ct_rfft32<12, true, true> is the one instantiation that carries a pack (sr_ct32.hip); a workgroup takes tiles b, b + series, ...:
    // more than two each and the pack is no longer a passenger
    return formulation == SR_CT_RFFT32 && F == 4096 && aligned != 0 && series >= 1 && tiles >= 1 && tiles <= 2 * series;
}

}  // extern "C"

// ---- the host path that the extensions of kernel 1 share: pair cross-correlation (sr_ct_cross*.hip), dipolar and dipolar pair function
// (sr_ct_dipolar*.hip), from device planes or resident vectors (sr_vectors.hip) --------------------------------------------------------
const sr_ct_form sr_ct_form_cross = {"two", 24, SR_CT_CROSS_LONG_FLOOR, "sr_ct_cross_long_f32_dev", true};
const sr_ct_form sr_ct_form_dipolar = {"four", 16, SR_CT_DIPOLAR_LONG_FLOOR, "sr_ct_dipolar_long_f32_dev", false};
const sr_ct_form sr_ct_form_dipolar_cross = {"eight", 32, SR_CT_DIPOLAR_CROSS_LONG_FLOOR, "sr_ct_dipolar_cross_long_f32_dev", true};
const sr_ct_form sr_ct_form_modes = {"five", 20, 0, nullptr, false};

size_t sr_ct_lds_bytes(int64_t F, int bytes_per_frame) { return (size_t)ct_Fp(F) * (size_t)bytes_per_frame; }

int64_t sr_ct_lds_max_frames(int bytes_per_frame, size_t lds_limit)
{
    int64_t F = (int64_t)lds_limit / bytes_per_frame - kPad;       // an upper bound: ct_Fp(F) >= F + kPad
    while (F >= 2 && sr_ct_lds_bytes(F, bytes_per_frame) > lds_limit) --F;
    return F >= 2 ? F : 0;
}

int sr_ct_chunks_check(const char *who, int64_t frames, int64_t R, int64_t F, const int64_t *chunk_start_host)
{
    if (chunk_start_host) {
        for (int64_t r = 0; r < R; ++r)
            SR_REQUIRE(chunk_start_host[r] >= 0 && chunk_start_host[r] + F <= frames, -3, "%s: chunk %lld start %lld out of range", who,
                       (long long)r, (long long)chunk_start_host[r]);
    } else {
        SR_REQUIRE(R * F <= frames, -3, "%s: R*F=%lld exceeds the %lld frames held", who, (long long)(R * F), (long long)frames);
    }
    return 0;
}

int sr_ct_rows_check(sr_ctx *ctx, const sr_ct_rows &w, const sr_ct_form &form)
{
    const char *who = w.who;
    if (form.pairs) {
        SR_REQUIRE(w.pair_i_host && w.pair_j_host, -2, "%s: null pointer", who);
        SR_REQUIRE(w.R >= 1 && w.F >= 2 && w.nV >= 1 && w.nP >= 1, -3, "%s: bad shape R=%lld F=%lld nV=%lld nP=%lld", who, (long long)w.R,
                   (long long)w.F, (long long)w.nV, (long long)w.nP);
        SR_REQUIRE((w.mode == 0 || w.mode == 1) && (w.sym == 0 || w.sym == 1), -3, "%s: mode and sym must be 0 or 1", who);
    } else {
        SR_REQUIRE(w.R >= 1 && w.F >= 2 && w.nV >= 1, -3, "%s: bad shape R=%lld F=%lld nV=%lld", who, (long long)w.R, (long long)w.F,
                   (long long)w.nV);
        SR_REQUIRE(w.mode == 0 || w.mode == 1, -3, "%s: mode must be 0 or 1", who);
    }
    if (w.blocked) {
        SR_REQUIRE(w.F <= SR_CT_LONG_MAX_FRAMES, -4, "%s: the blocked form takes chunks of at most %d frames, F=%lld", who, SR_CT_LONG_MAX_FRAMES,
                   (long long)w.F);
        SR_REQUIRE(w.F >= form.long_floor, -3, "%s: the blocked form takes chunks of at least %d frames, F=%lld", who, form.long_floor,
                   (long long)w.F);
    } else {
        const size_t limit = sr_lds_limit(ctx);
        SR_REQUIRE(sr_ct_lds_bytes(w.F, form.bytes_per_frame) <= limit, -4,
                   "%s: the %s series of a chunk of F=%lld frames need %zu B of LDS (> %zu); max F is %lld (longer chunks: %s%s)",
                   who, form.series, (long long)w.F, sr_ct_lds_bytes(w.F, form.bytes_per_frame), limit,
                   (long long)sr_ct_lds_max_frames(form.bytes_per_frame, limit), form.long_name ? "the blocked form, " : "this function has only the staged form",
                   form.long_name ? form.long_name : "");
    }
    const int64_t rows = form.pairs ? w.nP : w.nV;
    SR_REQUIRE(w.R * rows < (int64_t)1 << 30, -3, "%s: too many series", who);
    SR_REQUIRE((rows + kFinV - 1) / kFinV <= 65535, -3, "%s: too many %s in one call (%lld)", who, form.pairs ? "pairs" : "vectors",
               (long long)rows);                                   // k_ct_finalize's grid
    if (int rc = sr_ct_chunks_check(who, w.frames, w.R, w.F, w.chunk_start_host)) return rc;
    for (int64_t p = 0; form.pairs && p < w.nP; ++p)
        SR_REQUIRE(w.pair_i_host[p] >= 0 && w.pair_i_host[p] < w.nV && w.pair_j_host[p] >= 0 && w.pair_j_host[p] < w.nV, -3,
                   "%s: pair %lld = (%d, %d) is outside the %lld vectors", who, (long long)p, (int)w.pair_i_host[p], (int)w.pair_j_host[p],
                   (long long)w.nV);
    return 0;
}

double *sr_ct_psum(sr_ctx *ctx, double *psum_ws, int64_t rows, int64_t R, int64_t F)
{
    return psum_ws ? psum_ws : (double *)sr_workspace(ctx, SR_WS_PSUM, (size_t)(rows * R * sr_ct_psum_stride(F)) * sizeof(double));
}

namespace {

// what sr_ct_palmer_sums_f32_dev refuses, before anything is queued; *form: the formulation that runs
int ct_sums_check(sr_ctx *ctx, const char *who, const float *soa, int64_t Npad, int64_t R, int64_t F, int64_t nV,
                  const int64_t *chunk_start_host, int mode, const double *psum, int *form)
{
    SR_REQUIRE(soa && psum, -2, "%s: null pointer", who);
    SR_REQUIRE(R >= 1 && F >= 2 && nV >= 1, -3, "%s: bad shape R=%lld F=%lld nV=%lld", who, (long long)R, (long long)F, (long long)nV);
    SR_REQUIRE(mode == 0 || mode == 1, -3, "%s: mode must be 0 or 1", who);
    SR_REQUIRE(F <= SR_CT_LONG_MAX_FRAMES, -4, "%s: F=%lld frames per chunk; max F is %lld", who, (long long)F,
               (long long)SR_CT_LONG_MAX_FRAMES);
    *form = sr_ct_formulation(ctx->ct_fft, ctx->ct_long_min_frames, mode, F, (int64_t)sr_lds_limit(ctx));
    SR_REQUIRE(*form != SR_CT_REFUSED, -4,
               "%s: F=%lld frames per chunk need %zu B of LDS (> %zu) in the direct kernel (mode 1 or ct_fft < 2), "
               "whose max F is %lld; the default dispatch takes up to %lld",
               who, (long long)F, sr_ct_direct_lds_bytes(F), sr_lds_limit(ctx), (long long)sr_ct_direct_max_frames(sr_lds_limit(ctx)),
               (long long)SR_CT_LONG_MAX_FRAMES);
    SR_REQUIRE(R * nV < (int64_t)1 << 30, -3, "%s: too many series", who);
    if (chunk_start_host) {
        for (int64_t r = 0; r < R; ++r)
            SR_REQUIRE(chunk_start_host[r] >= 0 && chunk_start_host[r] + F <= Npad, -3, "%s: chunk %lld start %lld out of range", who,
                       (long long)r, (long long)chunk_start_host[r]);
    } else {
        SR_REQUIRE(R * F <= Npad, -3, "%s: R*F=%lld exceeds Npad=%lld", who, (long long)(R * F), (long long)Npad);
    }
    return 0;
}

// sr_ct_pack_fused on a checked pair of jobs
bool ct_carries(int form, const sr_ct_job &job, const sr_pack_job &next)
{
    const bool aligned = form == SR_CT_RFFT32 && sr_ct_rfft32_carries_pack(job) && (((uintptr_t)next.vecs | (uintptr_t)next.soa) & 15) == 0;
    return sr_ct_pack_fused(form, job.F, job.series, next.tiles, aligned) != 0;
}

sr_pack_job ct_next_job(const float *next_vecs, int64_t next_N, int64_t next_Vtot, int64_t next_v0, int64_t next_nV, float *next_soa,
                        int64_t next_Npad)
{
    const int64_t tiles = sr_pack_reg_tiles(next_Npad, next_Vtot, next_v0, next_nV);
    return {next_vecs, next_soa, next_N, next_Vtot, next_v0, next_Npad, (int)((next_Npad + 127) / 128),
            (int)(tiles < ((int64_t)1 << 30) ? tiles : 0)};
}

// what sr_ct_palmer_sums_pack_f32_dev refuses, before anything is queued
int ct_sums_pack_check(sr_ctx *ctx, const char *who, const float *soa, int64_t Npad, int64_t R, int64_t F, int64_t nV,
                       const int64_t *chunk_start_host, int mode, const double *psum, const float *next_vecs, int64_t next_N,
                       int64_t next_Vtot, int64_t next_v0, int64_t next_nV, const float *next_soa, int64_t next_Npad, int *form)
{
    if (int rc = sr_pack_soa_check(who, next_vecs, next_N, next_Vtot, next_v0, next_nV, next_soa, next_Npad)) return rc;
    if (int rc = ct_sums_check(ctx, who, soa, Npad, R, F, nV, chunk_start_host, mode, psum, form)) return rc;
    // the planes written must not be the planes read (nor the raw sums): whichever kernel packs, this launch reads `soa` to its end
    const uintptr_t s0 = (uintptr_t)soa, s1 = s0 + (size_t)(nV * 3 * Npad) * sizeof(float);
    const uintptr_t d0 = (uintptr_t)next_soa, d1 = d0 + (size_t)(next_nV * 3 * next_Npad) * sizeof(float);
    const uintptr_t p0 = (uintptr_t)psum, p1 = p0 + (size_t)(nV * R * sr_ct_psum_stride(F)) * sizeof(double);
    SR_REQUIRE((d1 <= s0 || s1 <= d0) && (d1 <= p0 || p1 <= d0), -3, "%s: the next batch's planes overlap this batch's planes or sums", who);
    return 0;
}

// stage the chunk starts and launch a checked job; `next` (optional): a pack for the same launch to carry when it can
// (sr_ct_pack_fused), else kernel 0 runs in front of it on the same stream
int ct_sums_launch(sr_ctx *ctx, const float *soa, int64_t Npad, int64_t R, int64_t F, int64_t nV, const int64_t *chunk_start_host,
                   int mode, double *psum, int form, const sr_pack_job *next, int64_t next_nV)
{
    int64_t *cs_dev = nullptr;
    if (chunk_start_host) {
        cs_dev = (int64_t *)sr_workspace(ctx, SR_WS_MISC, (size_t)R * sizeof(int64_t));
        if (!cs_dev) return -5;
        SR_HIP(hipMemcpyAsync(cs_dev, chunk_start_host, (size_t)R * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
        SR_HIP(hipStreamSynchronize(ctx->stream));      // tiny table: the caller's array is free again when this returns
    }
    const sr_ct_job job = {soa, Npad, chunk_start_host, cs_dev, psum, (int)R, (int)F, (int)(F / 2), (int)sr_ct_psum_stride(F), R * nV};
    if (next) {
        if (ct_carries(form, job, *next)) return sr_launch_ct_rfft32(ctx, job, next);
        if (int rc = sr_pack_soa_f32_dev(ctx, next->vecs, next->N, next->Vtot, next->v0, next_nV, next->soa, next->Npad)) return rc;
    }
    switch (form) {
        case SR_CT_DIRECT: return sr_launch_ct_direct(ctx, job, mode);
        case SR_CT_FFT64: return sr_launch_ct_fft64(ctx, job);
        case SR_CT_RFFT64: return sr_launch_ct_rfft64(ctx, job);
        case SR_CT_RFFT32: return sr_launch_ct_rfft32(ctx, job);
        default: return sr_launch_ct_long(ctx, job);
    }
}

}  // namespace

extern "C" {

int sr_ct_palmer_sums_f32_dev(sr_ctx *ctx, const float *soa, int64_t Npad, int64_t R, int64_t F, int64_t nV,
                              const int64_t *chunk_start_host, int mode, double *psum)
{
    SR_CHECK_CTX(ctx);
    int form;
    if (int rc = ct_sums_check(ctx, "sr_ct_palmer_sums_f32_dev", soa, Npad, R, F, nV, chunk_start_host, mode, psum, &form)) return rc;
    return ct_sums_launch(ctx, soa, Npad, R, F, nV, chunk_start_host, mode, psum, form, nullptr, 0);
}

int sr_ct_palmer_sums_pack_f32_dev(sr_ctx *ctx, const float *soa, int64_t Npad, int64_t R, int64_t F, int64_t nV,
                                   const int64_t *chunk_start_host, int mode, double *psum, const float *next_vecs, int64_t next_N,
                                   int64_t next_Vtot, int64_t next_v0, int64_t next_nV, float *next_soa, int64_t next_Npad)
{
    SR_CHECK_CTX(ctx);
    int form;
    if (int rc = ct_sums_pack_check(ctx, "sr_ct_palmer_sums_pack_f32_dev", soa, Npad, R, F, nV, chunk_start_host, mode, psum, next_vecs, next_N,
                                    next_Vtot, next_v0, next_nV, next_soa, next_Npad, &form))
        return rc;
    const sr_pack_job next = ct_next_job(next_vecs, next_N, next_Vtot, next_v0, next_nV, next_soa, next_Npad);
    return ct_sums_launch(ctx, soa, Npad, R, F, nV, chunk_start_host, mode, psum, form, &next, next_nV);
}

int sr_ct_palmer_sums_pack_plan(sr_ctx *ctx, const float *soa, int64_t Npad, int64_t R, int64_t F, int64_t nV,
                                const int64_t *chunk_start_host, int mode, const double *psum, const float *next_vecs, int64_t next_N,
                                int64_t next_Vtot, int64_t next_v0, int64_t next_nV, const float *next_soa, int64_t next_Npad)
{
    SR_CHECK_CTX(ctx);
    int form;
    if (int rc = ct_sums_pack_check(ctx, "sr_ct_palmer_sums_pack_plan", soa, Npad, R, F, nV, chunk_start_host, mode, psum, next_vecs, next_N,
                                    next_Vtot, next_v0, next_nV, next_soa, next_Npad, &form))
        return rc;
    const sr_ct_job job = {soa, Npad, chunk_start_host, nullptr, nullptr, (int)R, (int)F, (int)(F / 2), (int)sr_ct_psum_stride(F), R * nV};
    return ct_carries(form, job, ct_next_job(next_vecs, next_N, next_Vtot, next_v0, next_nV, const_cast<float *>(next_soa), next_Npad)) ? 1 : 0;
}

static int ct_finalize(sr_ctx *ctx, const double *psum, int64_t R, int64_t F, int64_t nV, double half, double *Ct, double *dCt, double *CtT,
                       double *dCtT)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(psum && Ct && dCt, -2, "sr_ct_finalize_f64_dev: null pointer");
    SR_REQUIRE((CtT == nullptr) == (dCtT == nullptr), -2, "sr_ct_finalize_t_f64_dev: CtT and dCtT go together");
    SR_REQUIRE(R >= 1 && F >= 2 && nV >= 1, -3, "sr_ct_finalize_f64_dev: bad shape");
    const int64_t L = F / 2;
    const int64_t Lp = sr_ct_psum_stride(F);
    const int64_t gx = (L + kFinD - 1) / kFinD, gy = (nV + kFinV - 1) / kFinV;
    SR_REQUIRE(gy <= 65535, -3, "sr_ct_finalize_f64_dev: too many vectors in one call (%lld)", (long long)nV);
    hipLaunchKernelGGL(k_ct_finalize, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, ctx->stream, psum, (int)R, (int)F, (int)L,
                       (int)Lp, nV, half, Ct, dCt, CtT, dCtT);
    SR_HIP(hipGetLastError());
    return 0;
}

int sr_ct_finalize_t_f64_dev(sr_ctx *ctx, const double *psum, int64_t R, int64_t F, int64_t nV, double *Ct, double *dCt,
                             double *CtT, double *dCtT)
{
    return ct_finalize(ctx, psum, R, F, nV, 0.5, Ct, dCt, CtT, dCtT);
}

}  // extern "C"

// internal (sr_internal.h): the finalizer of the distance-weighted functions
int sr_ct_finalize_weighted_f64_dev(sr_ctx *ctx, const double *psum, int64_t R, int64_t F, int64_t nV, double *Ct, double *dCt)
{
    return ct_finalize(ctx, psum, R, F, nV, 0.0, Ct, dCt, nullptr, nullptr);
}

extern "C" {

int sr_ct_finalize_f64_dev(sr_ctx *ctx, const double *psum, int64_t R, int64_t F, int64_t nV, double *Ct, double *dCt)
{
    return sr_ct_finalize_t_f64_dev(ctx, psum, R, F, nV, Ct, dCt, nullptr, nullptr);
}

int sr_ct_palmer_f32_dev(sr_ctx *ctx, const float *soa, int64_t Npad, int64_t R, int64_t F, int64_t nV,
                         const int64_t *chunk_start_host, int mode, double *psum_ws, double *Ct, double *dCt)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(soa && Ct && dCt, -2, "sr_ct_palmer_f32_dev: null pointer");
    SR_REQUIRE(R >= 1 && F >= 2 && nV >= 1, -3, "sr_ct_palmer_f32_dev: bad shape R=%lld F=%lld nV=%lld", (long long)R,
               (long long)F, (long long)nV);
    double *psum = psum_ws;
    if (!psum) {
        psum = (double *)sr_workspace(ctx, SR_WS_PSUM, (size_t)(nV * R * sr_ct_psum_stride(F)) * sizeof(double));
        if (!psum) return -5;
    }
    int rc = sr_ct_palmer_sums_f32_dev(ctx, soa, Npad, R, F, nV, chunk_start_host, mode, psum);
    if (rc) return rc;
    return sr_ct_finalize_f64_dev(ctx, psum, R, F, nV, Ct, dCt);
}

int sr_ct_palmer_f32(sr_ctx *ctx, const float *vecs, int64_t N, int64_t Vtot, int64_t v0, int64_t nV, int64_t R,
                     int64_t F, const int64_t *chunk_start_host, int mode, double *Ct, double *dCt)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(vecs && Ct && dCt, -2, "sr_ct_palmer_f32: null pointer");
    SR_REQUIRE(N > 0 && Vtot > 0 && nV > 0 && v0 >= 0 && v0 + nV <= Vtot, -3, "sr_ct_palmer_f32: bad shape");
    // the rank's columns [v0, v0 + nV) only: 12 N nV bytes over PCIe (sr_vectors.hip), then kernel 0 and kernel 1
    sr_vectors *h = sr_vectors_create(ctx, nV, N);
    if (!h) return -5;
    int rc = sr_vectors_append_f32(ctx, h, vecs, N, Vtot, v0);
    if (!rc) rc = sr_vectors_ct_f32(ctx, h, R, F, chunk_start_host, mode, Ct, dCt);
    sr_vectors_destroy(ctx, h);
    return rc;
}

}  // extern "C"
