// sr_ired_modes.hip -- iRED: the time-correlation functions of linear combinations ("modes") of the bond vectors' P2 tensors
//
//     A_mc(t) = sum_i e_mi u_ia(t) u_ib(t),                c = (a, b) over xx, yy, zz, xy, xz, yz          (amplitudes)
//     C_m(k)  = 1.5 / (F_w - k) sum_{tau < F_w - k} sum_c w_c A_mc(tau) A_mc(tau + k) - 0.5 sigma_m^2,     sigma_m = sum_i e_mi
//             = sum_ij e_mi e_mj < 1.5 (u_i(tau) . u_j(tau + k))^2 - 0.5 >_tau,       w = 1, 1, 1, 2, 2, 2
// per window w = frames [start, start + F_w) of the planes, lags k = 0 .. n_lags - 1 (Prompers & Brueschweiler, JACS 2002; Gu, Li &
// Brueschweiler, JCTC 2014).  With the rows of e the eigenvectors of that window's matrix M (sr_ired.hip), C_m(0) = lambda_m; the
// kernels take any (K, nV) matrix.  The literal definition: no unit-length assumption.
//
// k_ired_project: the GEMM D[m][(c, t)] = sum_i e_mi P_c(i, t) on the float64 matrix pipe, reduction over the vectors.  One workgroup
//   (4 waves) per (window, 64 modes, 64 frames), all six components; a wave owns 32 modes x 32 frames as 6 x 2 x 2 accumulators of
//   v_mfma_f64_16x16x4_f64.  One MFMA covers 4 vectors: lane l gives A[mode l & 15][vector l >> 4] = e and B[vector l >> 4][frame
//   l & 15] = u_a u_b, so a lane reads one coefficient, and x, y, z of ONE vector at ONE frame (float32, LDS), and forms the six
//   operands in registers: a product of two float32 values is exact in float64, the only rounding is the accumulation.
//   LDS holds kVS = 16 vectors of a stage: coefficients [mode][vector] in rows of 17 doubles, planes [vector][component][frame] with
//   a vector 208 floats on (4 vectors x 16 frames of a read fall on 64 different banks); the next stage is fetched into registers
//   while the current one is multiplied.  Modes past K, vectors past nV and frames past the window are staged as zeros, which add
//   exactly 0.  The whole reduction of an output block runs in one workgroup in the order of the vectors: no atomics, no split, the
//   amplitudes are a function of the input alone.
//   The accumulator map of the f64 instruction is col = lane & 15, row = (lane >> 4) + 4 reg (NOT the f32 one).
//   Output: amp[window of the batch][m][c][t], t < F_w contiguous.
// k_ired_mode_ct: k_ct_fft's scheme (sr_ct_fft64.hip) on the six amplitude series of one (window, mode): three packed complex pairs
//   (xx, yy), (zz, xy), (xz, yz) with weights 1,1 / 1,2 / 2,2, the weighted power spectrum, one transform back; transform length
//   M = 2048 / 4096 / 6144 / 8192, the smallest >= F_w + n_lags - 1.  sigma_m is summed in float64 in a fixed order.
#include "sr_fft64.h"
#include <vector>

namespace {

constexpr int kMT = 64;                        // modes per tile
constexpr int kFT = 64;                        // frames per tile
constexpr int kVS = 16;                        // vectors per LDS stage: a multiple of 4 (one MFMA k-step)
constexpr int kCoefRow = kVS + 1;              // doubles per staged mode
constexpr int kVecRow = 3 * kFT + 16;          // floats per staged vector (banks, see above)
constexpr int kCoefPer = kMT * kVS / 256;      // 4 coefficients and
constexpr int kPlanePer = kVS * 3 * kFT / 256; // 12 plane samples per thread and stage
constexpr int kWinCols = 3;                    // window table: start, length, offset of the window's amplitudes (in doubles)
constexpr int kMaxNeed = 8192;                 // longest transform
static_assert(kMT * kVS % 256 == 0 && kVS * 3 * kFT % 256 == 0 && kVS % 4 == 0 && kVecRow % 64 == 16, "stage shape");

typedef double d4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_ired_project(const float *__restrict__ soa, int64_t Npad, int nV, const int64_t *__restrict__ win,
                                                      const double *__restrict__ coef, int K, double *__restrict__ amp)
{
    __shared__ double lc[kMT * kCoefRow];
    __shared__ float lp[kVS * kVecRow];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = blockIdx.z, m0 = blockIdx.y * kMT;
    const int64_t start = win[kWinCols * w], len = win[kWinCols * w + 1];
    const int64_t t0 = (int64_t)blockIdx.x * kFT;
    if (t0 >= len) return;                                 // the grid is sized by the longest window of the batch (the whole workgroup leaves)
    const double *cw = coef + (int64_t)w * K * nV;

    // what this thread fetches of every stage; -1 = a mode past K / a frame past the window
    int64_t csrc[kCoefPer], psrc[kPlanePer];
    int cv[kCoefPer], pv[kPlanePer], cdst[kCoefPer], pdst[kPlanePer];
#pragma unroll
    for (int q = 0; q < kCoefPer; ++q) {
        const int idx = tid + 256 * q, m = idx / kVS;
        cv[q] = idx - m * kVS;
        cdst[q] = m * kCoefRow + cv[q];
        csrc[q] = m0 + m < K ? (int64_t)(m0 + m) * nV : -1;
    }
#pragma unroll
    for (int q = 0; q < kPlanePer; ++q) {
        const int idx = tid + 256 * q, row = idx / kFT, t = idx - row * kFT;
        pv[q] = row / 3;
        const int c = row - 3 * pv[q];
        pdst[q] = pv[q] * kVecRow + c * kFT + t;
        psrc[q] = t0 + t < len ? (int64_t)c * Npad + start + t0 + t : -1;
    }
    double cpre[kCoefPer];
    float ppre[kPlanePer];
    auto fetch = [&](int v0) {
#pragma unroll
        for (int q = 0; q < kCoefPer; ++q) cpre[q] = (csrc[q] >= 0 && v0 + cv[q] < nV) ? cw[csrc[q] + v0 + cv[q]] : 0.0;
#pragma unroll
        for (int q = 0; q < kPlanePer; ++q)
            ppre[q] = (psrc[q] >= 0 && v0 + pv[q] < nV) ? soa[(int64_t)(v0 + pv[q]) * 3 * Npad + psrc[q]] : 0.f;
    };

    d4 acc[6][2][2];
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int h = 0; h < 2; ++h) acc[c][g][h] = d4{0.0, 0.0, 0.0, 0.0};

    // this lane's operand sources: mode (lane & 15) of the wave's two 16-mode groups, frame (lane & 15) of its two 16-frame groups,
    // vector lane >> 4 of a k-step
    const int wr = wave >> 1, wc = wave & 1, lv = lane & 15, lk = lane >> 4;
    const double *ap[2];
    const float *bp[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        ap[g] = lc + (wr * 32 + g * 16 + lv) * kCoefRow + lk;
        bp[g] = lp + lk * kVecRow + wc * 32 + g * 16 + lv;
    }

    fetch(0);
    for (int v0 = 0; v0 < nV; v0 += kVS) {
        __syncthreads();                                   // the previous stage has been read
#pragma unroll
        for (int q = 0; q < kCoefPer; ++q) lc[cdst[q]] = cpre[q];
#pragma unroll
        for (int q = 0; q < kPlanePer; ++q) lp[pdst[q]] = ppre[q];
        __syncthreads();
        if (v0 + kVS < nV) fetch(v0 + kVS);                // in flight during the products below
#pragma unroll
        for (int k = 0; k < kVS / 4; ++k) {
            double A[2], B[2][6];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                A[g] = ap[g][4 * k];
                const float *b = bp[g] + 4 * k * kVecRow;
                const double x = b[0], y = b[kFT], z = b[2 * kFT];
                B[g][0] = x * x; B[g][1] = y * y; B[g][2] = z * z;
                B[g][3] = x * y; B[g][4] = x * z; B[g][5] = y * z;
            }
#pragma unroll
            for (int c = 0; c < 6; ++c)
#pragma unroll
                for (int g = 0; g < 2; ++g)
#pragma unroll
                    for (int h = 0; h < 2; ++h) acc[c][g][h] = __builtin_amdgcn_mfma_f64_16x16x4f64(A[g], B[h][c], acc[c][g][h], 0, 0, 0);
        }
    }

    // f64 accumulator map: col = lane & 15 (frame), row = (lane >> 4) + 4 reg (mode)
    double *out = amp + win[kWinCols * w + 2];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wr * 32 + g * 16 + lk + 4 * r;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int64_t t = t0 + wc * 32 + h * 16 + lv;
                if (m < K && t < len)
#pragma unroll
                    for (int c = 0; c < 6; ++c) out[((int64_t)m * 6 + c) * len + t] = acc[c][g][h][r];
            }
        }
}

struct ModeCtArgs {
    const double *amp;            // amplitudes of the batch
    const int64_t *win;           // the batch's rows of the window table
    const double *coef;           // (Wb, K, nV)
    const Ct64Tab *tab;
    double *Cm;                   // (Wb, K, n_lags)
    int K, nV, n_lags;
};

// N1 of the transform a window takes: M = 256 N1 is the smallest length >= need = F_w + n_lags - 1
__host__ __device__ inline int ired_n1(int64_t need) { return need <= 2048 ? 8 : need <= 4096 ? 16 : need <= 6144 ? 24 : 32; }

// one workgroup per (window, mode); the windows of a launch whose transform length is not 256 N1 are left to the launch of theirs
template <int N1>
__global__ __launch_bounds__(256) void k_ired_mode_ct(ModeCtArgs a)
{
    extern __shared__ __align__(16) unsigned char fft_smem[];
    cplx *lds = reinterpret_cast<cplx *>(fft_smem);
    constexpr int M = N1 * 256;
    constexpr int G = N1 / 8;
    const int tid = threadIdx.x;
    const int w = blockIdx.x / a.K, m = blockIdx.x - w * a.K;
    const int F = (int)a.win[kWinCols * w + 1];
    if (ired_n1((int64_t)F + a.n_lags - 1) != N1) return;
    const double *series = a.amp + a.win[kWinCols * w + 2] + (int64_t)m * 6 * F;
    cplx *fb = lds + tid + (tid >> 3);                 // frequency / natural order: element tid + 256 j + 32 N1 k'

    double W[G][8];
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) W[j][e] = 0.0;

    // three packed pairs: (xx, yy) weights 1,1; (zz, xy) weights 1,2; (xz, yz) weights 2,2
#pragma unroll 1
    for (int pair = 0; pair < 3; ++pair) {
        asm volatile("" ::: "memory");
        const double *pp = series + (int64_t)(2 * pair) * F, *pq = pp + F;
        // unconditional loads from a clamped index + select, all issued before the first use (see k_ct_fft)
        cplx sig[N1];
#pragma unroll
        for (int n1 = 0; n1 < N1; ++n1) {
            const int n = tid + 256 * n1;
            const bool in = n < F;
            const int nc = in ? n : 0;
            const double pv = pp[nc], qv = pq[nc];
            sig[n1] = {in ? pv : 0.0, in ? qv : 0.0};
        }
        cplx w8[G][8];
        fft_workgroup<N1>(sig, w8, lds, a.tab, tid);
        // spectrum to LDS in frequency order, then every thread reads the mirror frequency of its own ones
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int p = 0; p < 8; ++p) fb[fft_pad(256 * j + 32 * N1 * bitrev<3>(p))] = w8[j][p];
        __syncthreads();
        const double wp = pair == 2 ? 2.0 : 1.0, wq = pair == 0 ? 1.0 : 2.0;
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int k = tid + 256 * j + 32 * N1 * bitrev<3>(p);
                const int km = k == 0 ? 0 : M - k;
                const cplx zm = lds[km + (km >> 3) + 8 * (km >> 8)];
                const cplx zk = w8[j][p];
                // P = (Z(k) + conj Z(M-k)) / 2, Q = (Z(k) - conj Z(M-k)) / (2i)
                const double sr = zk.re + zm.re, si = zk.im - zm.im;
                const double dr = zk.re - zm.re, di = zk.im + zm.im;
                W[j][p] += 0.25 * (wp * (sr * sr + si * si) + wq * (dr * dr + di * di));
            }
        __syncthreads();
    }
    // the weighted power spectrum (real, even) back through the same transform
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
        for (int p = 0; p < 8; ++p) fb[fft_pad(256 * j + 32 * N1 * bitrev<3>(p))] = {W[j][p], 0.0};
    __syncthreads();
    {
        cplx sig[N1];
#pragma unroll
        for (int n1 = 0; n1 < N1; ++n1) sig[n1] = fb[fft_pad(256 * n1)];
        __syncthreads();
        cplx w8[G][8];
        fft_workgroup<N1>(sig, w8, lds, a.tab, tid);
        // sigma_m = sum_i e_mi in a fixed order: thread t adds i = t, t + 256, ...; the wave sums (sr_wave_sum_f64) are added as
        // (0 + 1) + (2 + 3).  The transform above ended with a barrier: its LDS is free
        double sigma;
        {
            const double *e = a.coef + ((int64_t)w * a.K + m) * a.nV;
            double part = 0.0;
            for (int i = tid; i < a.nV; i += 256) part += e[i];
            part = sr_wave_sum_f64(part);
            double *red = reinterpret_cast<double *>(fft_smem);
            if ((tid & 63) == 0) red[tid >> 6] = part;
            __syncthreads();
            sigma = (red[0] + red[1]) + (red[2] + red[3]);
        }
        double *out = a.Cm + ((int64_t)w * a.K + m) * a.n_lags;
        const double inv = 1.0 / (double)M, half_s2 = 0.5 * sigma * sigma;
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int lag = tid + 256 * j + 32 * N1 * bitrev<3>(p);
                if (lag < a.n_lags) out[lag] = 1.5 * (w8[j][p].re * inv) / (double)(F - lag) - half_s2;
            }
    }
}

template <int N1>
int launch_mode_ct(sr_ctx *ctx, const ModeCtArgs &a, int64_t blocks)
{
    return sr_launch(ctx, k_ired_mode_ct<N1>, dim3((unsigned)blocks), dim3(256), (size_t)fft_lds_slots(256 * N1) * sizeof(cplx), a);
}

}  // namespace

// the argument checks of both entry points: `frames` are the frames a window may reach (Npad of the planes, or the frames held)
int sr_ired_mode_ct_check(const char *who, int64_t frames, int64_t nV, const int64_t *win_start_host, const int64_t *win_len_host, int W, int K,
                          int n_lags)
{
    SR_REQUIRE(nV >= 1 && W >= 1 && frames >= 1, -3, "%s: bad shape nV=%lld W=%d frames=%lld", who, (long long)nV, W, (long long)frames);
    SR_REQUIRE(nV <= 32768, -3, "%s: nV=%lld vectors; at most 32768", who, (long long)nV);
    SR_REQUIRE(K >= 1 && K <= 32768, -3, "%s: K=%d modes; 1 .. 32768", who, K);
    SR_REQUIRE(n_lags >= 1, -3, "%s: n_lags=%d; at least 1", who, n_lags);
    for (int w = 0; w < W; ++w) {
        const int64_t a = win_start_host[w], n = win_len_host[w];
        SR_REQUIRE(n >= 1, -3, "%s: window %d has length %lld", who, w, (long long)n);
        SR_REQUIRE(a >= 0 && a <= frames && n <= frames - a, -3, "%s: window %d = frames [%lld, %lld) is outside the %lld held", who, w,
                   (long long)a, (long long)(a + n), (long long)frames);
        SR_REQUIRE(n_lags <= n, -3, "%s: n_lags=%d exceeds the %lld frames of window %d", who, n_lags, (long long)n, w);
        SR_REQUIRE(n + n_lags - 1 <= kMaxNeed, -4, "%s: window %d: win_len + n_lags - 1 = %lld + %d - 1 exceeds %d, the longest transform", who,
                   w, (long long)n, n_lags, kMaxNeed);
    }
    return 0;
}

extern "C" {

int sr_ired_mode_ct_f32_dev(sr_ctx *ctx, const float *soa, int64_t Npad, int64_t nV, const int64_t *win_start_host,
                            const int64_t *win_len_host, int W, const double *coef_dev, int K, int n_lags, double *Cm_dev)
{
    SR_CHECK_CTX(ctx);
    SR_REQUIRE(soa && win_start_host && win_len_host && coef_dev && Cm_dev, -2, "sr_ired_mode_ct_f32_dev: null pointer");
    if (int rc = sr_ired_mode_ct_check("sr_ired_mode_ct_f32_dev", Npad, nV, win_start_host, win_len_host, W, K, n_lags)) return rc;
    // ---- batches of consecutive windows whose amplitudes (6 K F_w doubles each) fit the work area; at least one window each ----
    const int64_t budget = (int64_t)ctx->ired_ws_mb << 20;
    std::vector<int64_t> table((size_t)W * kWinCols);
    std::vector<int> first;                                 // first window of every batch, and W behind the last
    int64_t used = 0, area = 0;
    for (int w = 0; w < W; ++w) {
        const int64_t bytes = 6 * (int64_t)K * win_len_host[w] * (int64_t)sizeof(double);
        if (w == 0 || used + bytes > budget || w - first.back() >= 65535 || (int64_t)(w - first.back() + 1) * K >= (int64_t)1 << 31) {
            first.push_back(w);
            used = 0;
        }
        table[kWinCols * w] = win_start_host[w];
        table[kWinCols * w + 1] = win_len_host[w];
        table[kWinCols * w + 2] = used / (int64_t)sizeof(double);
        used += bytes;
        if (used > area) area = used;
    }
    first.push_back(W);
    int64_t *win_dev = (int64_t *)sr_workspace(ctx, SR_WS_MISC, table.size() * sizeof(int64_t));
    double *amp = (double *)sr_workspace(ctx, SR_WS_IRED_AMP, (size_t)area);
    const Ct64Tab *tab = (const Ct64Tab *)sr_ct64_table(ctx);
    if (!win_dev || !amp || !tab) return -5;
    SR_HIP(hipMemcpyAsync(win_dev, table.data(), table.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    SR_HIP(hipStreamSynchronize(ctx->stream));          // tiny table: the caller's arrays are free again when this returns
    // ---- per batch: the projection, then the transforms of every transform length the batch holds ----
    for (size_t b = 0; b + 1 < first.size(); ++b) {
        const int w0 = first[b], Wb = first[b + 1] - w0;
        int64_t Fb = 0;
        bool has[4] = {false, false, false, false};
        for (int w = w0; w < w0 + Wb; ++w) {
            if (win_len_host[w] > Fb) Fb = win_len_host[w];
            has[ired_n1(win_len_host[w] + n_lags - 1) / 8 - 1] = true;
        }
        const int64_t *wt = win_dev + (int64_t)kWinCols * w0;
        const double *cb = coef_dev + (int64_t)w0 * K * nV;
        if (int rc = sr_launch(ctx, k_ired_project, dim3((unsigned)((Fb + kFT - 1) / kFT), (unsigned)((K + kMT - 1) / kMT), (unsigned)Wb), dim3(256),
                               0, soa, Npad, (int)nV, wt, cb, K, amp))
            return rc;
        ModeCtArgs a;
        a.amp = amp; a.win = wt; a.coef = cb; a.tab = tab; a.Cm = Cm_dev + (int64_t)w0 * K * n_lags;
        a.K = K; a.nV = (int)nV; a.n_lags = n_lags;
        const int64_t blocks = (int64_t)Wb * K;
        int rc = 0;
        if (!rc && has[0]) rc = launch_mode_ct<8>(ctx, a, blocks);
        if (!rc && has[1]) rc = launch_mode_ct<16>(ctx, a, blocks);
        if (!rc && has[2]) rc = launch_mode_ct<24>(ctx, a, blocks);
        if (!rc && has[3]) rc = launch_mode_ct<32>(ctx, a, blocks);
        if (rc) return rc;
    }
    return 0;
}

}  // extern "C"
