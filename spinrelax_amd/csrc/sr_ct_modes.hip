// sr_ct_modes.hip -- the bond-vector correlation function split into the five tumbling modes of an anisotropic diffusion tensor
// (k_ct_modes), an extension beyond the reference, whose anisotropic J(w) multiplies a static orientation histogram by one internal
// C(t): sr_noe_modes' definition (sr_noe.hip) with w = 1, at every lag of a chunk of kernel 1's Palmer chunk table.
//
// Definition.  u(t) the unit bond vector rotated by the constant F = R(q_F) into the principal-axis frame of the tensor; five signals
//     s0 = u_z^2 - 1/3,  s1 = u_x^2 - u_y^2,  s2 = u_y u_z,  s3 = u_x u_z,  s4 = u_x u_y
// and per chunk of F frames and lag k = 0 .. L = F / 2, with <.> = sum_t / (F - k) over the origins t with t + k inside the chunk and
// the primed signal taken at t + k:
//     H0 = <s0 s0'>,  H1 = <s1 s1'>,  H2 = <s0 s1' + s1 s0'> / 2,  H3 = <s2 s2'>,  H4 = <s3 s3'>,  H5 = <s4 s4'>
// 2.25 H0 + 0.75 H1 + 3 (H3 + H4 + H5) is kernel 1's C(k) whatever the frame; the amplitudes of the five modes of a tensor D are host
// work (spinrelax_amd/noe.py: mode_amplitudes; spinrelax_amd/modes.py).
//
// Kernels:
//   k_pack_modes        frame-major vectors of any positive length -> five planes per vector s0 .. s4 in kernel 0's layout
//                       (soa[(v * 5 + c) * Npad + n], zero for n in [N, Npad)); F and the normalisation in float64, each value rounded
//                       once to float32; a vector with a frame that is not finite or of zero length gets bad[v] = 1 (a plain store of
//                       the same value by whoever meets one: no atomics); the tile transpose is pack_planes_tile (sr_pack_planes.h)
//   k_ct_modes<W>       one (vector, chunk) per workgroup or per slab of one (the scaffold and the launch ladder of sr_ct_staged.h): the five series staged
//                       as k_ct_dipolar stages its w series (sr_ct_dipolar.h), 20 bytes per frame; per lag block the seven shifted-product
//                       sums (0,0) (1,1) (0,1) (1,0) (2,2) (3,3) (4,4) by seven calls of dip_shift_block_w, one sum at a time so that
//                       only one set of float64 accumulators lives beside the inner loop: float32 FMAs, float32 partial sums of at most
//                       16 signed terms started at zero, folded into float64; remaining lags and every lag in mode 1 by a float64 path;
//                       while staging, wave 0 of slab 0 sums the five signals of the chunk in float64.  No atomics, no scratch: equal
//                       input gives bit-equal output, and nothing depends on the other vectors of a call
//   k_ct_modes_finalize mean and std / (sqrt(R) - 1) over the chunks of S / (F - k), kernel 1's convention (k_ct_finalize) without its
//                       1.5 S' - 0.5, lag 0 included; the means of the five signals
// Why seven calls and not one fused block: docs/EXPERIMENTS.md section 37.
// A chunk must fit 20 ct_Fp(F) bytes of LDS: F <= 7968 at 160 KiB.  Longer chunks would take a blocked form.
#include "sr_ct_dipolar.h"
#include "sr_ct_staged.h"
#include "sr_pack_planes.h"
#include "sr_noe_host.h"
#include <cmath>

namespace {

// ------------------------------------------------------------------------------------------
// the five-plane pack
// ------------------------------------------------------------------------------------------
constexpr int kModeSig = 5;             // signals per vector
constexpr int kModeSums = 6;            // sums per (vector, chunk, lag)
constexpr int kModeFinV = 16;           // vectors per workgroup of k_ct_modes_finalize: k_ct_finalize's, whose grid sr_ct_rows_check bounds

struct ModeFrame {
    double m[9];                        // F, row-major
};

__global__ __launch_bounds__(256) void k_pack_modes(const float *__restrict__ vecs, int64_t N, int64_t Vtot, int64_t v0, int64_t nV,
                                                    const ModeFrame fr, float *__restrict__ soa, int64_t Npad, int32_t *__restrict__ bad)
{
    pack_planes_tile<kModeSig>(vecs, N, Vtot, v0, nV, soa, Npad, [=](const float *p, int64_t, int64_t v, float (&o)[kModeSig]) {
#pragma clang fp contract(off)
        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
        const double len = sqrt(x * x + y * y + z * z);
        if (!(len > 0.0) || isinf(len)) {
            bad[v] = 1;
        } else {
            const double ux = (fr.m[0] * x + fr.m[1] * y + fr.m[2] * z) / len;
            const double uy = (fr.m[3] * x + fr.m[4] * y + fr.m[5] * z) / len;
            const double uz = (fr.m[6] * x + fr.m[7] * y + fr.m[8] * z) / len;
            o[0] = (float)(uz * uz - 1.0 / 3.0);
            o[1] = (float)(ux * ux - uy * uy);
            o[2] = (float)(uy * uz);
            o[3] = (float)(ux * uz);
            o[4] = (float)(ux * uy);
        }
    });
}

// ------------------------------------------------------------------------------------------
// the correlation kernel
// ------------------------------------------------------------------------------------------
#ifndef SR_CT_MODES_WAVES_EU
#define SR_CT_MODES_WAVES_EU 3
#endif
template <int W>
__global__ __launch_bounds__(W * 64, SR_CT_MODES_WAVES_EU) void k_ct_modes(CtStagedArgs a)     // soa (nV, 5, Npad); psum (nV, R, 6, Lp): slot k holds lag k; sums = ssum (nV, R, 5)
{
    extern __shared__ __align__(16) float lds[];
    const int Fp = a.Fp, Hw = Fp >> 1, F = a.F, Lp = a.Lp;
    const CtWorker w = ct_worker<W>(a, a.nslab);
    const int tid = w.tid, lane = w.lane;

    // ---- stage the five series, series c at lds + c Fp (coalesced dword loads; zero padding behind frame F) ----
    {
        const float *p = a.soa + (int64_t)w.row * kModeSig * a.Npad + ct_chunk_start(a, w);
        for (int e = tid; e < Fp; e += W * 64) {
            const int pos = lds_wpos(e, Hw);
            const bool in = e < F;
#pragma unroll
            for (int c = 0; c < kModeSig; ++c) lds[c * Fp + pos] = in ? p[(int64_t)c * a.Npad + e] : 0.f;
        }
    }
    __syncthreads();

    // ---- the sums of the five signals over the chunk, float64, fixed order ----
    if (w.slab == 0 && w.wave == 0) {
        double s[kModeSig];
#pragma unroll
        for (int c = 0; c < kModeSig; ++c) s[c] = 0.0;
        for (int t = lane; t < F; t += 64) {
            const int pos = lds_wpos(t, Hw);
#pragma unroll
            for (int c = 0; c < kModeSig; ++c) s[c] += (double)lds[c * Fp + pos];
        }
#pragma unroll
        for (int c = 0; c < kModeSig; ++c) {
            s[c] = wave_sum_f64(s[c]);
            if (lane == 0) a.sums[((int64_t)w.row * a.R + w.r) * kModeSig + c] = s[c];
        }
    }

    const int nb = ct_full_blocks(a);
    const int NW = ct_workers<W>(a.nslab), wid = ct_worker_id<W>(w);
    double *out = ct_psum_row(a, w, kModeSums * Lp);

    // ---- fast path: full lag blocks (lag 0 included) ----
    ct_for_each_lag_block(nb, NW, wid, lane, [=](int dw, int g, int l16) SR_CT_INLINE {
        // one sum at a time: (0,0) | (1,1) | (0,1) + (1,0) | (2,2) | (3,3) | (4,4)
#pragma unroll 1
        for (int c = 0; c < kModeSums; ++c) {
            double acc[kLagsPerLane];
            ct_zero_lags(acc);
            const int sa = c < 2 ? c : (c == 2 ? 0 : c - 1), sb = c < 2 ? c : (c == 2 ? 1 : c - 1);     // earlier and later series
            dip_shift_block_w(lds + sa * Fp, lds + sb * Fp, Hw, F, dw, g, l16, acc, 0.f);
            if (c == 2) dip_shift_block_w(lds + Fp, lds, Hw, F, dw, g, l16, acc, 0.f);
            ct_combine_strips(acc, l16);
            if (g == 0) {
                double *o = ct_lag_slots(out + (int64_t)c * Lp, dw, l16);
#pragma unroll
                for (int d = 0; d < kLagsPerLane; ++d) o[d] = c == 2 ? 0.5 * acc[d] : acc[d];
            }
        }
    });

    // ---- float64 path: remaining lags (and every lag in validation mode) ----
    ct_tail_lags<kModeSums>(nb * kLagBlock, a.L, F, NW, wid, lane, [=](int j, int d, double (&s)[kModeSums]) SR_CT_INLINE {
        const int pa = lds_wpos(j, Hw), pb = lds_wpos(j + d, Hw);
        double x[kModeSig], y[kModeSig];
#pragma unroll
        for (int c = 0; c < kModeSig; ++c) {
            x[c] = (double)lds[c * Fp + pa];
            y[c] = (double)lds[c * Fp + pb];
        }
        s[0] += x[0] * y[0];
        s[1] += x[1] * y[1];
        s[2] += x[0] * y[1] + x[1] * y[0];
        s[3] += x[2] * y[2];
        s[4] += x[3] * y[3];
        s[5] += x[4] * y[4];
    }, [=](int d, const double (&s)[kModeSums]) SR_CT_INLINE {
#pragma unroll
        for (int c = 0; c < kModeSums; ++c) out[(int64_t)c * Lp + d] = c == 2 ? 0.5 * s[c] : s[c];
    });
}

// H, dH (L + 1, nV, 6): mean over the R chunks of S / (F - k) and its std / (sqrt(R) - 1), numpy.std's two passes in chunk order as
// k_ct_finalize takes them; smean (nV, 5): the chunk sums of the signals added in chunk order, over R F.  A wave reads 64 consecutive
// lags of one (vector, chunk, sum).
__global__ __launch_bounds__(256) void k_ct_modes_finalize(const double *__restrict__ psum, const double *__restrict__ ssum, int R, int F, int L,
                                                           int Lp, int64_t nV, double *__restrict__ H, double *__restrict__ dH,
                                                           double *__restrict__ smean)
{
    const int tid = threadIdx.x;
    const int d = blockIdx.x * 64 + (tid & 63);         // the lag
    const double n = (double)(F - d);
    const double rootR = sqrt((double)R) - 1.0;
    const int64_t stride = (int64_t)kModeSums * Lp;
#pragma unroll 1
    for (int i = 0; i < kModeFinV / 4; ++i) {
        const int64_t v = (int64_t)blockIdx.y * kModeFinV + (tid >> 6) + 4 * i;
        if (v >= nV) break;
        if (blockIdx.x == 0 && (tid & 63) < kModeSig) {
            const int c = tid & 63;
            double m = 0.0;
            for (int r = 0; r < R; ++r) m += ssum[(v * R + r) * kModeSig + c];
            smean[v * kModeSig + c] = m / ((double)R * (double)F);
        }
        if (d > L) continue;
#pragma unroll 1
        for (int c = 0; c < kModeSums; ++c) {
            const double *p = psum + (v * R * kModeSums + c) * Lp + d;
            double m = 0.0, s = 0.0;
            for (int r = 0; r < R; ++r) m += p[r * stride] / n;
            m /= (double)R;
            for (int r = 0; r < R; ++r) {
                const double e = p[r * stride] / n - m;
                s += e * e;
            }
            const int64_t o = ((int64_t)d * nV + v) * kModeSums + c;
            H[o] = m;
            dH[o] = sqrt(s / (double)R) / rootR;
        }
    }
}

}  // namespace

extern "C" {

int64_t sr_ct_modes_max_frames(sr_ctx *ctx)
{
    if (!ctx) return -1;
    return sr_ct_lds_max_frames(sr_ct_form_modes.bytes_per_frame, sr_lds_limit(ctx));
}

int sr_pack_modes_f32_dev(sr_ctx *ctx, const float *vecs, int64_t N, int64_t Vtot, int64_t v0, int64_t nV, const double *frame_quat_host,
                          float *planes, int64_t Npad, int32_t *bad)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(vecs && planes && bad, -2, "sr_pack_modes_f32_dev: null pointer");
    dim3 grid;
    if (int rc = pack_planes_grid("sr_pack_modes_f32_dev", N, Vtot, v0, nV, Npad, grid)) return rc;
    ModeFrame fr;
    char msg[160];
    if (int rc = noe_frame_matrix(frame_quat_host, fr.m, msg, sizeof msg)) {
        sr_set_error("sr_pack_modes_f32_dev: %s", msg);
        return rc;
    }
    SR_HIP(hipMemsetAsync(bad, 0, (size_t)nV * sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(k_pack_modes, grid, dim3(256), 0, ctx->stream, vecs, N, Vtot, v0, nV, fr, planes, Npad, bad);
    SR_HIP(hipGetLastError());
    return 0;
}

int sr_ct_modes_f32_dev(sr_ctx *ctx, const float *planes, int64_t Npad, int64_t nV, int64_t R, int64_t F, const int64_t *chunk_start_host,
                        int mode, double *psum_ws, double *H, double *dH, double *smean)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(planes && H && dH && smean, -2, "sr_ct_modes_f32_dev: null pointer");
    const sr_ct_rows w = {"sr_ct_modes_f32_dev", Npad, nV, R, F, chunk_start_host, nullptr, nullptr, 0, 0, mode, 0};
    if (int rc = sr_ct_rows_check(ctx, w, sr_ct_form_modes)) return rc;
    const int64_t L = F / 2, Lp = sr_ct_psum_stride(F);
    double *psum = sr_ct_psum(ctx, psum_ws, kModeSums * nV, R, F);
    if (!psum) return -5;
    // ---- stage the chunk starts; the chunk sums of the five signals live behind them ----
    sr_stage st(ctx);
    const int64_t *cs_dev = sr_ct_stage_tables(st, w, kModeSig * (size_t)(nV * R) * sizeof(double)).chunk_start;
    CtStagedArgs a = ct_staged_args(planes, Npad, cs_dev, psum, R, F, mode);
    a.sums = st.take<double>(kModeSig * (size_t)(nV * R));
    if (int rc = chunk_start_host ? st.finish() : st.rc) return rc;     // tiny table: the caller's array is free again when this returns
    if (int rc = ct_launch_slabs(ctx, k_ct_modes<1>, k_ct_modes<4>, a, R * nV, sr_ct_form_modes.bytes_per_frame)) return rc;
    hipLaunchKernelGGL(k_ct_modes_finalize, dim3((unsigned)((L + 1 + 63) / 64), (unsigned)((nV + kModeFinV - 1) / kModeFinV)), dim3(256), 0, ctx->stream, psum, a.sums,
                       (int)R, (int)F, (int)L, (int)Lp, nV, H, dH, smean);
    SR_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
