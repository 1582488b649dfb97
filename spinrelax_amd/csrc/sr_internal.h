// sr_internal.h -- shared declarations of libspinrelax_hip.so (not part of the public ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../include/spinrelax_hip.h"

#define SR_NSLOTS 22

struct sr_ctx {
    int device;
    hipStream_t stream;
    hipDeviceProp_t prop;
    hipEvent_t ev0, ev1;
    // growable device workspaces, one per purpose, reused across calls (no hipMalloc in steady state)
    void *slot[SR_NSLOTS];
    size_t slot_bytes[SR_NSLOTS];
    // tuning (sr_set_option)
    int fit_waves;      // waves per residue in the model-order search: 1, 2 or 4
    int fit_geo;        // 1 (default): on a uniform time grid the fit kernels form exp(-t/tau) of a thread's points by multiplication
                        // (sr_fit.hip, Residue::stage); 0: exp() per point whatever the grid
    int fit_lds;        // 1: stage t, y, 1/sigma of a residue in LDS when it fits; 0: read them from global memory
    int ct_fft;         // formulation of kernel 1, 0 .. 4 (default 3): one input of sr_ct_formulation(), whose rule is written out at
                        // the top of sr_ct.hip
    int ct_wg_per_cu;   // k_ct_rfft32: at most this many workgroups per CU (0 = as many as fit: 4 for M = 6144); see sr_ct32.hip
    int ct_traceless;   // 1: k_ct_rfft<12> in its traceless five-signal form (faster alone, slower inside the pipeline: default 0)
    int ct_long_ws_mb;  // blocked C(t) (sr_ct_long.hip): the series of a launch go in tiles whose block spectra fit this many MiB
    int ct_long_min_frames;   // blocked C(t): beyond one transform (F + L > 8192), chunks of at least this many frames take it, and the
                        // shorter ones that the direct kernel cannot stage; default SR_CT_LONG_MIN_FRAMES
    int ct_cross_long_min_frames;   // pair cross-correlation: spinrelax_amd/ct.py gives chunks of at least this many frames to the blocked form
                        // (sr_ct_cross_long.hip); the library's entry points do not dispatch, each runs its own kernel
    int ct_dipolar_long_min_frames, ct_dipolar_cross_long_min_frames;   // the same for the two distance-weighted functions
                        // (sr_ct_dipolar_long.hip)
    int ired_ksplit;   // iRED matrix (sr_ired.hip): workgroups that share a window's frames per tile pair; 0 (default) = sr_ired_ksplit()'s rule
    int ired_ws_mb;     // iRED mode correlation functions (sr_ired_modes.hip): the windows of a call go in batches whose amplitudes fit this many MiB
    int fft_table_ready;
    int fft32_table_ready;
    int ctlong_table_ready;
    hipEvent_t ctlong_ev;   // behind the last kernel of the latest blocked C(t) call: the next call, on whatever stream, waits for it
    int ctlong_ev_set;      // before it touches the work area
    // strided host -> device copies of bond vectors (sr_vectors.hip): two pinned staging buffers, and what went through them
    void *stage[2];
    hipEvent_t stage_ev[2];
    int stage_busy[2];
    unsigned long long h2d_bytes, h2d_calls;
};

enum {
    SR_WS_VECS = 0,     // staged host vectors (frame-major)
    SR_WS_SOA,          // packed planes
    SR_WS_PSUM,         // C(t) raw sums
    SR_WS_OUT0, SR_WS_OUT1, SR_WS_OUT2, SR_WS_OUT3,
    SR_WS_IN0, SR_WS_IN1, SR_WS_IN2, SR_WS_IN3,
    SR_WS_MISC,
    SR_WS_FIT,          // residual work space of the fit kernel (when the caller passes none)
    SR_WS_FFT,          // twiddle table of the FFT formulation of kernel 1
    SR_WS_FFT32,        // tables of its float32 form (sr_ct32.hip)
    SR_WS_CTLONG,       // blocked C(t) (sr_ct_long.hip): chunk constants, block spectra and cross-spectra of one tile of series
    SR_WS_CTLONG_TAB,   // twiddles of its float64 inverse transform
    SR_WS_IRED,         // iRED matrix (sr_ired.hip): partial tiles of the frame split, (W, tile pairs, S, 64 x 64) float64
    SR_WS_IRED_AMP,     // iRED mode correlation functions (sr_ired_modes.hip): amplitudes of one batch of windows, (m, 6, F_w) float64 each
    SR_WS_NOE,          // all-pairs dipolar map (sr_noe.hip): partial tiles of the frame split, (B, S, tile pairs, T x T, 7) float64; those of its lagged and mode-resolved forms
    SR_WS_SYMM,         // symmetric product (sr_noesy.hip): partial tiles of the k split, (S, tile pairs, 64 x 64) float64
    SR_WS_EXPM          // matrix exponential (sr_noesy.hip): the scaled matrix Y (P, P) and the P row sums of |R|
};

void sr_set_error(const char *fmt, ...);
void *sr_workspace(sr_ctx *ctx, int slot, size_t bytes);   // returns NULL (error set) on failure

#define SR_HIP(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            sr_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return -100 - (int)e_;                                                          \
        }                                                                                   \
    } while (0)

#define SR_CHECK_CTX(ctx)                                                                   \
    do {                                                                                    \
        if (!(ctx)) { sr_set_error("null sr_ctx"); return -1; }                            \
        SR_HIP(hipSetDevice((ctx)->device));                                                \
    } while (0)

#define SR_REQUIRE(cond, code, ...)                                                         \
    do {                                                                                    \
        if (!(cond)) { sr_set_error(__VA_ARGS__); return (code); }                          \
    } while (0)

// largest LDS allocation one workgroup may ask for (160 KiB on gfx950)
static inline size_t sr_lds_limit(const sr_ctx *ctx)
{
    size_t a = ctx->prop.maxSharedMemoryPerMultiProcessor, b = ctx->prop.sharedMemPerBlock;
    return a > b ? a : b;
}

// allow the kernel `func` to be launched with `bytes` (> 64 KiB) of dynamic LDS on this context's device.  That permission
// is a per-DEVICE attribute of ONE function: the largest size granted so far is remembered per (device, function pointer) for
// the whole PROCESS (monotonic, under a lock; sr_core.hip), so two contexts on one device can never lower each other's grant,
// and every instance of a kernel template has its own.  The only caller is sr_launch below.
int sr_grant_lds(sr_ctx *ctx, const void *func, size_t bytes);

static inline int64_t sr_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// ---- kernel 1: the formulations behind sr_ct_palmer_sums_f32_dev (sr_ct.hip chooses, see its header) ------------------------
constexpr int kLagBlock = 128;          // lags per wave pass of the direct kernel, which writes whole blocks: the slack of sr_ct_psum_stride

// what every launcher below gets: R chunks of F frames of nV vectors, raw lag sums out
struct sr_ct_job {
    const float *soa;                   // packed planes, Npad floats each
    int64_t Npad;
    const int64_t *cs_host, *cs_dev;    // chunk starts, the same R values on the host and on the device; both null: chunk r starts at r F
    double *psum;                       // (nV, R, Lp)
    int R, F, L, Lp;
    int64_t series;                     // R nV
    int planes = 3;                     // planes per vector in soa; 4: the dipolar pack a_x, a_y, a_z, w (sr_launch_ct_long only)
    int traceless = 0;                  // sr_launch_ct_long only: the five traceless signals whatever |a| is (sr_ct_dipolar_long.hip)
};

// sr_ct_direct.hip: shifted products (k_ct_palmer); mode as in sr_ct_palmer_sums_f32_dev.  The series is staged in LDS, so the
// caller checks sr_ct_direct_lds_bytes(F) against sr_lds_limit() first; the longest F that a limit admits is for messages.
int sr_launch_ct_direct(sr_ctx *ctx, const sr_ct_job &job, int mode);
size_t sr_ct_direct_lds_bytes(int64_t F);
int64_t sr_ct_direct_max_frames(size_t lds_limit);

// sr_ct_fft64.hip: float64 transforms in LDS, complex (k_ct_fft: 1024 < F + L <= 8192) and real-input (k_ct_rfft: 4096 < F + L <= 8192)
int sr_launch_ct_fft64(sr_ctx *ctx, const sr_ct_job &job);
int sr_launch_ct_rfft64(sr_ctx *ctx, const sr_ct_job &job);

// ---- the extensions of kernel 1: pair cross-correlation, dipolar and dipolar pair function, each staged (LDS) and blocked.  Their
// entry points share one host path (sr_ct.hip): null checks, sr_ct_rows_check, sr_ct_psum, sr_ct_stage_tables, launch, epilogue ----
// what an entry point is asked for: R chunks of F frames out of the `frames` held, of nV vectors or of nP pairs of them
struct sr_ct_rows {
    const char *who;                            // the entry point, for messages
    int64_t frames, nV, R, F;
    const int64_t *chunk_start_host;            // null: chunk r starts at r F
    const int32_t *pair_i_host, *pair_j_host;   // [nP]; the autocorrelation form has none (nP = 0): its rows are the nV vectors
    int64_t nP;
    int sym, mode, blocked;
};
// what tells the three functions apart on the host
struct sr_ct_form {
    const char *series;                         // "two", "four", "eight": the series a workgroup of the staged form holds in LDS,
    int bytes_per_frame;                        // and their bytes per staged frame
    int long_floor;                             // the shortest chunk of the blocked form
    const char *long_name;                      // and its entry point, for the staged form's -4 message; null: the staged form is the only one
    bool pairs;                                 // rows are pairs (a pair table is required) or the vectors themselves
};
extern const sr_ct_form sr_ct_form_cross, sr_ct_form_dipolar, sr_ct_form_dipolar_cross;
extern const sr_ct_form sr_ct_form_modes;       // the mode-resolved function (sr_ct_modes.hip): five signal series, staged form only
// LDS of a staged chunk of F frames, and the longest chunk that a limit admits (0: none)
size_t sr_ct_lds_bytes(int64_t F, int bytes_per_frame);
int64_t sr_ct_lds_max_frames(int bytes_per_frame, size_t lds_limit);
// what the entry points refuse, before any workspace is requested or anything is queued: a missing pair table (-2), shapes, mode and
// sym (-3), a chunk whose series do not fit the LDS (-4; blocked: a chunk of more than SR_CT_LONG_MAX_FRAMES frames, and -3 below the
// form's floor), too many rows for one call, chunk starts and pair indices outside the frames / vectors held (-3)
int sr_ct_rows_check(sr_ctx *ctx, const sr_ct_rows &w, const sr_ct_form &form);
int sr_ct_chunks_check(const char *who, int64_t frames, int64_t R, int64_t F, const int64_t *chunk_start_host);
// raw sums (rows, R, sr_ct_psum_stride(F)): the caller's work area, or the context's when there is none; NULL (error set) on failure
double *sr_ct_psum(sr_ctx *ctx, double *psum_ws, int64_t rows, int64_t R, int64_t F);

// sr_ct_cross.hip: k_ct_cross_p0 on raw sums (nP, R, sr_ct_psum_stride(F)) whose slot 0 holds lag 0: P0 (nP) the chunk mean of
// 1.5 S / F - half and, when dP0 is not null, its std / (sqrt(R) - 1); device arrays, asynchronous on ctx->stream.  half: 0.5 for unit
// vectors, 0 for the distance-weighted raw sums S_a - S_w / 3
int sr_ct_cross_p0_dev(sr_ctx *ctx, const double *psum, int64_t R, int64_t F, int64_t nP, double half, double *P0, double *dP0);

// sr_ct.hip: sr_ct_finalize_f64_dev for the distance-weighted raw sums S_a - S_w / 3 (sr_ct_dipolar.hip): mean and std / (sqrt(R) - 1)
// over the chunks of 1.5 S / (F - k), nothing subtracted
int sr_ct_finalize_weighted_f64_dev(sr_ctx *ctx, const double *psum, int64_t R, int64_t F, int64_t nV, double *Ct, double *dCt);

// sr_ct_cross_long.hip: the blocked form of the pair cross-correlation (raw sums in kernel 1's layout, lag 0 in slot 0), for what
// sr_ct_rows_check(blocked = 1) admits: the range in which the kernels it shares with sr_ct_long.hip are tested
#define SR_CT_CROSS_LONG_FLOOR 5462
#define SR_CT_CROSS_LONG_MIN_FRAMES 6625   /* default of "ct_cross_long_min_frames": the first length k_ct_cross cannot stage */
// A checked job whose tables the caller has put on `st` (sr_ct_stage_tables with room for 2 nP more int32 behind them): the launcher
// appends its two slot tables and calls st->finish(), on every path.  ct: psum (nP, R, Lp), series = R nP, and planes = 3,
// traceless = 0 for unit-vector planes (sr_ct_cross.hip) or planes = 4, traceless = 1 for the dipolar pack: five traceless signals and
// S_a - S_w / 3 in slot 0 (sr_ct_dipolar_long.hip, mode 0 only)
struct sr_stage;
struct sr_ct_pair_job {
    sr_ct_job ct;
    int64_t nV, nP;
    const int32_t *pair_i_host, *pair_j_host, *pair_i_dev, *pair_j_dev;
    int sym, mode;
    sr_stage *st;
};
int sr_launch_ct_cross_long(sr_ctx *ctx, const sr_ct_pair_job &job);

// sr_ct_dipolar_long.hip: the blocked forms of both, on planes from sr_pack_dipolar_f32_dev.  The floors are the shortest chunks at
// which the shared kernels keep a block structure they are tested at (5462: F + L > 8192; 4097: two blocks, one offset)
#define SR_CT_DIPOLAR_LONG_FLOOR 5462
#define SR_CT_DIPOLAR_LONG_MIN_FRAMES 10017        /* default of "ct_dipolar_long_min_frames": the first length k_ct_dipolar cannot stage */
#define SR_CT_DIPOLAR_CROSS_LONG_FLOOR 4097
#define SR_CT_DIPOLAR_CROSS_LONG_MIN_FRAMES 4897   /* default of "ct_dipolar_cross_long_min_frames": the first k_ct_dipolar_cross cannot stage */
// sr_ct_dipolar.hip, sr_ct_dipolar_cross.hip: the normalising kernels behind k_ct_finalize (and k_ct_cross_p0), shared with the blocked forms
int sr_ct_dipolar_norm_dev(sr_ctx *ctx, const double *wsum, int64_t R, int64_t F, int64_t nV, double *Ct, double *dCt, double *wmean);
int sr_ct_dipolar_cross_norm_dev(sr_ctx *ctx, const double *wsum2, int64_t R, int64_t F, int64_t nP, double *Ct, double *dCt, double *P0,
                                 double *dP0);

// sr_ired_modes.hip
#define SR_IRED_WS_MB 1024
int sr_ired_mode_ct_check(const char *who, int64_t frames, int64_t nV, const int64_t *win_start_host, const int64_t *win_len_host, int W, int K,
                          int n_lags);

// sr_ct32.hip: float32 real-input transforms in LDS (k_ct_rfft32: 1024 < F + L <= 8192).  With `pk` the launch also carries the pack of
// the next batch (sr_pack_tile.h), which only the cfg3 / cfg4 instantiation does: ask sr_ct_rfft32_carries_pack(job) first
struct sr_pack_job;
int sr_launch_ct_rfft32(sr_ctx *ctx, const sr_ct_job &job, const sr_pack_job *pk = nullptr);
bool sr_ct_rfft32_carries_pack(const sr_ct_job &job);
// sr_pack.hip: what sr_pack_soa_f32_dev refuses (null pointers -2, shapes -3), before anything is queued
int sr_pack_soa_check(const char *who, const float *vecs, int64_t N, int64_t Vtot, int64_t v0, int64_t nV, const float *soa, int64_t Npad);

// the device tables of the float32 transforms (Ct32Tab[4], sr_ct32_fft.h), created on first use; NULL (error set) on failure
const void *sr_ct32_tables(sr_ctx *ctx);

// sr_ct_long.hip: blocked float32 transforms for chunks that do not fit one in-LDS transform (F + L > 8192), up to
// SR_CT_LONG_MAX_FRAMES frames per chunk
#define SR_CT_LONG_MAX_FRAMES 262144
#define SR_CT_LONG_MIN_FRAMES 16384     /* default of "ct_long_min_frames": above what the direct kernel can stage (about 13400 frames), i.e. the
                                           direct kernel keeps every chunk it can stage (no timing of the two against each other exists yet) */
#define SR_CT_LONG_WS_MB 256
int sr_launch_ct_long(sr_ctx *ctx, const sr_ct_job &job);

#ifdef __HIPCC__
// ---- the one way to launch a kernel that takes dynamic LDS ------------------------------------------
// grants `lds` first when it is above the 64 KiB every kernel may have, launches on ctx->stream, returns the launch's status
template <class... KArgs, class... Args>
inline int sr_launch(sr_ctx *ctx, void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, Args &&...args)
{
    if (lds > 64 * 1024)
        if (int rc = sr_grant_lds(ctx, reinterpret_cast<const void *>(kernel), lds)) return rc;
    hipLaunchKernelGGL(kernel, grid, block, lds, ctx->stream, args...);
    SR_HIP(hipGetLastError());
    return 0;
}
#endif

// ---- staging of the host-pointer entry points -------------------------------------------------------
// A bump allocator over one workspace slot at a time, with copies in stream order on ctx->stream: open() names the slot and
// its size, take() carves (aligned to the element type), put() carves and copies host -> device, fetch() copies device -> host,
// finish() waits for the stream.  The FIRST failure is kept -- the code and sr_set_error text that sr_workspace / SR_HIP give
// -- and turns every later call into a no-op that returns null: an entry point tests `rc` once before it launches, and
// returns finish().  A null host pointer is an optional array that is absent: put() returns null for it, fetch() skips it.
struct sr_stage {
    sr_ctx *ctx;
    char *p = nullptr, *end = nullptr;
    int rc = 0;

    explicit sr_stage(sr_ctx *c) : ctx(c) {}
    sr_stage &open(int slot, size_t bytes)
    {
        if (rc) return *this;
        p = (char *)sr_workspace(ctx, slot, bytes);
        end = p + bytes;
        if (!p) rc = -5;
        return *this;
    }
    template <class T>
    T *take(size_t n)
    {
        char *q = p + (size_t)(-(uintptr_t)p & (alignof(T) - 1));
        if (rc) return nullptr;
        if (!p || n * sizeof(T) > (size_t)(end - q)) return (T *)fail(hipErrorInvalidValue, "sr_stage::take past the end of the slot");
        p = q + n * sizeof(T);
        return (T *)q;
    }
    template <class T>
    T *take(int slot, size_t n) { return open(slot, n * sizeof(T)).template take<T>(n); }     // an array with a slot of its own
    template <class T>
    T *put(const T *host, size_t n)
    {
        T *d = host ? take<T>(n) : nullptr;
        if (d) fail(hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(host to device)");
        return rc ? nullptr : d;
    }
    template <class T>
    void fetch(T *host, const T *dev, size_t n)
    {
        if (host && !rc) fail(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(device to host)");
    }
    int finish()
    {
        if (!rc) fail(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
        return rc;
    }
    void *fail(hipError_t e, const char *what)
    {
        if (e != hipSuccess && !rc) {
            sr_set_error("%s: %s -> %s", __FILE__, what, hipGetErrorString(e));
            rc = -100 - (int)e;
        }
        return nullptr;
    }
};

// the tables of a C(t) extension on the device: chunk starts (null: regular chunks) and, in the pair forms, the pair table
struct sr_ct_tables {
    const int64_t *chunk_start;
    const int32_t *pair_i, *pair_j;
};
// opens SR_WS_MISC for them with `room` bytes behind for the caller to take() and queues the copies; the caller tests st.rc or calls
// st.finish(), which also frees the caller's arrays again
inline sr_ct_tables sr_ct_stage_tables(sr_stage &st, const sr_ct_rows &w, size_t room)
{
    st.open(SR_WS_MISC, (size_t)w.R * sizeof(int64_t) + 2 * (size_t)w.nP * sizeof(int32_t) + room);
    sr_ct_tables t;
    t.chunk_start = st.put(w.chunk_start_host, (size_t)w.R);
    t.pair_i = st.put(w.pair_i_host, (size_t)w.nP);
    t.pair_j = st.put(w.pair_j_host, (size_t)w.nP);
    return t;
}

#ifdef __HIPCC__
// ---- wave-level float64 sum on the VALU only (DPP + readlane), no LDS round trips -----------------
// __shfl_xor on a double compiles to two ds_bpermute_b32 per step (LDS crossbar, ~100 cycles of
// dependent latency each); the fit kernel reduces 54 values per Jacobian and was parked on those waits
// half of its life (rocprofv3: SQ_WAIT_ANY 51 %).  DPP moves are ordinary VALU instructions.
__device__ __forceinline__ double sr_dpp_f64(double v, const int ctrl_sel)
{
    union { double d; int i[2]; } a, b;
    a.d = v;
    switch (ctrl_sel) {
        case 0:  // quad_perm [1,0,3,2]
            b.i[0] = __builtin_amdgcn_update_dpp(0, a.i[0], 0xB1, 0xF, 0xF, true);
            b.i[1] = __builtin_amdgcn_update_dpp(0, a.i[1], 0xB1, 0xF, 0xF, true);
            break;
        case 1:  // quad_perm [2,3,0,1]
            b.i[0] = __builtin_amdgcn_update_dpp(0, a.i[0], 0x4E, 0xF, 0xF, true);
            b.i[1] = __builtin_amdgcn_update_dpp(0, a.i[1], 0x4E, 0xF, 0xF, true);
            break;
        case 2:  // row_half_mirror
            b.i[0] = __builtin_amdgcn_update_dpp(0, a.i[0], 0x141, 0xF, 0xF, true);
            b.i[1] = __builtin_amdgcn_update_dpp(0, a.i[1], 0x141, 0xF, 0xF, true);
            break;
        default:  // row_mirror
            b.i[0] = __builtin_amdgcn_update_dpp(0, a.i[0], 0x140, 0xF, 0xF, true);
            b.i[1] = __builtin_amdgcn_update_dpp(0, a.i[1], 0x140, 0xF, 0xF, true);
            break;
    }
    return b.d;
}

__device__ __forceinline__ double sr_readlane_f64(double v, int lane)
{
    union { double d; int i[2]; } a, b;
    a.d = v;
    b.i[0] = __builtin_amdgcn_readlane(a.i[0], lane);
    b.i[1] = __builtin_amdgcn_readlane(a.i[1], lane);
    return b.d;
}

// sum over the 64 lanes of a wave, result identical in every lane; fixed association order
__device__ __forceinline__ double sr_wave_sum_f64(double v)
{
    v += sr_dpp_f64(v, 0);
    v += sr_dpp_f64(v, 1);
    v += sr_dpp_f64(v, 2);
    v += sr_dpp_f64(v, 3);            // every lane of a 16-lane row holds the row sum
    const double r0 = sr_readlane_f64(v, 0), r1 = sr_readlane_f64(v, 16);
    const double r2 = sr_readlane_f64(v, 32), r3 = sr_readlane_f64(v, 48);
    return (r0 + r1) + (r2 + r3);
}

// ---- many sums at once: NV values per lane -> lane L ends up with the 64-lane total of value bitrev6(L) ------------
// Reducing NV values one by one costs NV x (4 DPP steps + 8 readlanes + 3 adds) ~ 25 instructions each; the fit kernel's
// Jacobian reduces 54 (J^T J and J^T f at n = 9): 1 350 instructions per wave, a third of the Jacobian pass itself.
// Here every level HALVES the number of live registers instead: for a pair of values (a, b), the lanes whose level bit is
// 0 keep a and receive the partner lane's a, the others keep b and receive the partner's b -- one exchange and one add
// turn two registers into one.  54 -> 27 -> 14 -> 7 -> 4 -> 2 -> 1 registers: ~220 instructions.
//   level 1, 2: lane bits 5 and 4 with v_permlane32_swap / v_permlane16_swap (gfx950: swap the upper half / the odd
//               rows of one register with the lower half / the even rows of the other: 2 instructions per double)
//   level 3, 4: bits 3 and 2 inside a 16-lane row: row_mirror / row_half_mirror DPP moves under bank masks
//   level 5, 6: bits 1 and 0 inside a quad: quad_perm DPP moves + per-lane selects
// Association order (fixed, the same for every value): lanes are paired l <-> l+32, then rows r <-> r^1, then i <-> 15-i
// inside a row, i <-> 7-i inside its halves, i <-> 3-i inside its quads, finally neighbours.  A missing partner value
// (odd count) is 0, which adds exactly.
template <int CTRL, int BANK_MASK>
__device__ __forceinline__ int sr_dpp_i32(int old, int src)
{
    return __builtin_amdgcn_update_dpp(old, src, CTRL, 0xF, BANK_MASK, false);
}

template <int LEVEL>
__device__ __forceinline__ double sr_reduce_pair(double a, double b, int lane)
{
    union U { double d; int i[2]; unsigned u[2]; };
    U ua, ub, k, t;
    ua.d = a; ub.d = b;
    if (LEVEL == 1) {            // after the swap: ua = [a.lo32, b.lo32], ub = [a.hi32, b.hi32]
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            auto r = __builtin_amdgcn_permlane32_swap(ua.u[h], ub.u[h], false, false);
            ua.u[h] = r[0]; ub.u[h] = r[1];
        }
        return ua.d + ub.d;
    } else if (LEVEL == 2) {     // rows: ua = [a0, b0, a2, b2], ub = [a1, b1, a3, b3]
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            auto r = __builtin_amdgcn_permlane16_swap(ua.u[h], ub.u[h], false, false);
            ua.u[h] = r[0]; ub.u[h] = r[1];
        }
        return ua.d + ub.d;
    } else if (LEVEL == 3 || LEVEL == 4) {
        constexpr int ctrl = LEVEL == 3 ? 0x140 : 0x141;            // row_mirror / row_half_mirror
        constexpr int m0 = LEVEL == 3 ? 0x3 : 0x5, m1 = LEVEL == 3 ? 0xC : 0xA;   // banks whose level bit is 0 / 1
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            t.i[h] = sr_dpp_i32<ctrl, m0>(0, ua.i[h]);               // bit 0 lanes: the partner's a
            t.i[h] = sr_dpp_i32<ctrl, m1>(t.i[h], ub.i[h]);          // bit 1 lanes: the partner's b
            k.i[h] = sr_dpp_i32<0xE4, m1>(ua.i[h], ub.i[h]);         // keep a (bit 0 lanes) or b (bit 1 lanes)
        }
        return k.d + t.d;
    } else {
        constexpr int ctrl = LEVEL == 5 ? 0x1B : 0xB1;               // quad_perm [3,2,1,0] / [1,0,3,2]
        const bool bit = (lane & (LEVEL == 5 ? 2 : 1)) != 0;
        U s;
        k.d = bit ? b : a;
        s.d = bit ? a : b;
#pragma unroll
        for (int h = 0; h < 2; ++h) t.i[h] = sr_dpp_i32<ctrl, 0xF>(0, s.i[h]);
        return k.d + t.d;
    }
}

template <int LEVEL, int N>
__device__ __forceinline__ void sr_reduce_level(double *v, int lane)
{
#pragma unroll
    for (int m = 0; m < (N + 1) / 2; ++m) v[m] = sr_reduce_pair<LEVEL>(v[2 * m], 2 * m + 1 < N ? v[2 * m + 1] : 0.0, lane);
}

// v[0 .. NV) per lane, NV <= 64 (destroyed); returns the total of value sr_reduced_index(lane) (garbage when that index
// is >= NV)
template <int NV>
__device__ __forceinline__ double sr_wave_sum_many_f64(double *v, int lane)
{
    constexpr int N1 = (NV + 1) / 2, N2 = (N1 + 1) / 2, N3 = (N2 + 1) / 2, N4 = (N3 + 1) / 2, N5 = (N4 + 1) / 2;
    sr_reduce_level<1, NV>(v, lane);
    sr_reduce_level<2, N1>(v, lane);
    sr_reduce_level<3, N2>(v, lane);
    sr_reduce_level<4, N3>(v, lane);
    sr_reduce_level<5, N4>(v, lane);
    sr_reduce_level<6, N5>(v, lane);
    return v[0];
}
__device__ __forceinline__ int sr_reduced_index(int lane) { return (int)(__builtin_bitreverse32((unsigned)lane) >> 26); }
#endif
