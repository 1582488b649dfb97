/*
 * spinrelax_hip.h -- C ABI of libspinrelax_hip.so: the MI355X (gfx950) implementation of SpinRelax's
 * bond-vector autocorrelation -> spectral density -> R1/R2/NOE hot path.
 *
 * The reference (zharmad/SpinRelax) has no FFI for this path: its boundary is four CLI scripts,
 * their file formats, a handful of Python functions and ONE native symbol, the numpy ufunc
 * npufunc.Jomega (Jomega/Jomega.c:30-156).  Each entry point below names the reference
 * function (file:line, relative to the reference root) whose work it replaces; INTEGRATION.md shows
 * the ctypes binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - every function returns int: 0 = ok, negative = error; text via sr_last_error();
 *   - plain pointers and sizes only; "_dev" entry points take DEVICE pointers and enqueue work on the
 *     context's stream without synchronising (outputs are valid after sr_sync or a stream sync);
 *     entry points without "_dev" take HOST pointers, stage through the context's workspace and
 *     block until the result is in the caller's buffer;
 *   - one sr_ctx per GPU per thread; no internal locking; no callbacks or exceptions cross the ABI;
 *   - the context owns growable work areas (raw C(t) sums, histogram counters, staging buffers).  They are
 *     tied to no stream: sr_pack_soa*, sr_ct_palmer_f32_dev, sr_rotate_hist_f32_dev and every host-pointer entry
 *     point must be issued on ONE stream at a time (sr_set_stream between them is fine once the previous work is
 *     ordered before the next, e.g. same stream).  sr_expfit_order_search_f64_dev (with its `work` argument),
 *     sr_expfit_lm_f64_dev (ditto), sr_jomega_relax_f64_dev and sr_transpose_f64_dev use caller memory only and
 *     may run on several streams at once -- that is how spinrelax_amd/pipeline.py overlaps batches;
 *   - small HOST tables handed to "_dev" entry points (atom index lists, lag lists, chunk starts, a quaternion, bin edges)
 *     are validated before anything is queued and are consumed when the call returns: the caller may free them at once;
 *   - there is no CPU fallback: without a gfx950 device sr_create fails.
 */
#ifndef SPINRELAX_HIP_H
#define SPINRELAX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sr_ctx sr_ctx;

#define SR_ABI_VERSION 13   /* unchanged by the sr_ct_cross, sr_ct_dipolar, sr_ct_dipolar_cross, sr_ct_dipolar_long, sr_noe and sr_noesy entry points: they only add symbols, and a binding that meets an older library fails at the missing symbol */

/* ---- context, memory, timing ------------------------------------------------------------- */
int          sr_abi_version(void);
/* sha256 (hex, first 16 characters) of the sources and compiler flags this library was built from (spinrelax_amd/build.py
 * computes it and compiles it in); "unknown" for a build that bypassed build.py.  bench.py compares it with the id stored
 * in the committed PMC profile to tell whether per-launch counter figures still belong to the kernels that ran. */
const char  *sr_build_id(void);
const char  *sr_last_error(void);
sr_ctx      *sr_create(int device);                 /* NULL on failure (see sr_last_error)        */
void         sr_destroy(sr_ctx *);
int          sr_set_stream(sr_ctx *, void *hip_stream);   /* hipStream_t; NULL = default stream  */
int          sr_sync(sr_ctx *);
/* Tuning knobs: "fit_waves" = wavefronts per residue in the fits (1, 2 or 4; default 2: four workgroups per CU -- the
 * model-order search is then limited by its registers alone -- and the shortest time per batch with the chip full, 0.40 ms for the
 * 512-residue benchmark batch against 0.60 at 4 and 0.82 at 1; a lone launch lasts 6.9 ms at 2, 6.3 at 4, 24.7 at 1; results are
 * bit-identical only between runs with the same value), "fit_lds" = 1/0 keep
 * a residue's t, C(t), 1/sigma in LDS, "fit_geo" = 1/0 (default 1): when a residue's time axis is a uniform grid (t[l] = t[0] + l dt
 * to 1.8e-15 relative -- checked per residue on the device; any other axis always takes exp() per point) the fit kernels form
 * exp(-t/tau) at the points a thread owns by multiplication, exp() once per thread: a point j products past its thread's exp()
 * (j < L / (64 fit_waves): up to 15 at L = 2048 and two waves) is within ((3 + 3 j) + 12 t/tau) u of exp(-t/tau), u = 2^-53 (exp()
 * per point: (3 + 2 t/tau) u), 17 % less time per batch
 * with the chip full; 0 = exp() per point whatever the axis, "ct_fft" = formulation of kernel 1 for the chunks that fit one transform
 * in LDS, 1024 < F + L <= 8192: 3 (default) the
 * FLOAT32 real-input FFT for 4096 < F + L <= 8192 (the reference's own arithmetic type; C(t) to 6e-8 of C(0) on ordered vectors,
 * 1.6e-7 on tumbling or jumping ones) and the float64 complex
 * FFT below, 4 float32 transforms at every such length, 2 the float64 real-input FFT for 4096 < F + L <= 8192 (C(t) to
 * 1e-15) and the complex one below, 1 the float64 complex FFT at every such length, 0 always direct; 2 and more also admit the
 * blocked transforms for longer chunks (sr_ct_formulation() below is the rule itself);
 * "ct_traceless" = 1/0 (default 0): the real-input FFT kernel for F <= 4096 transforms the five traceless components of
 * u (x) u and takes the trace term from a scan of |u|^2 - 1 (one transform fewer; series that are not unit vectors fall back
 * to six inside the kernel) -- 4 % faster alone, 3 % slower per step inside the pipeline, same results to 1e-13;
 * "ired_ksplit" = S >= 1: the iRED matrix kernel splits every window's frames over S workgroups per tile pair; 0 (default): the
 * rule of sr_ired_matrix_f32_dev below, a function of the shape alone.  M is bit-equal between runs with the same value;
 * "ired_ws_mb" = MiB (1 .. 65536, default 1024): sr_ired_mode_ct_f32_dev processes its windows in batches whose amplitudes fit this
 * work area (a batch always holds at least one window); the results do not depend on it. */
int          sr_set_option(sr_ctx *, const char *name, int value);
/* Streams that partition the chip.  The fits of fitting_Ct_functions.py:278-345 are a latency chain of small
 * launches; queued behind a C(t) launch that fills every CU they starve (queue priority does not pre-empt
 * resident workgroups).  sr_stream_create returns a hipStream_t whose kernels may only run on the CUs whose bit is
 * set in cu_mask (n_words 32-bit words, bit i of word w = CU 32*w+i in the runtime's numbering; NULL / 0 words =
 * all CUs); priority as hipStreamCreateWithPriority (lower = more urgent, 0 = default). */
int          sr_stream_create(sr_ctx *, const uint32_t *cu_mask, int n_words, int priority, void **stream_out);
int          sr_stream_destroy(sr_ctx *, void *hip_stream);
/* Signals: 32-bit values in memory that a KERNEL (or sr_stream_write_signal) sets and a stream waits for without the host
 * (hipStreamWaitValue32 on hipMallocSignalMemory).  sr_stream_wait_signal holds back everything queued afterwards on the
 * context's stream until *sig >= value; always pair a kernel-side release with an sr_stream_write_signal of the same value
 * behind that kernel, so that the wait ends at the latest when the kernel has finished.  NULL when the device cannot do it.
 * ORDERING RULE (enforced): the release must be SUBMITTED before the wait is queued -- first the releasing launch and its
 * sr_stream_write_signal(sig, v) on their stream, then sr_stream_wait_signal(sig, v) on the waiting stream.  Streams of one
 * priority share a few hardware queues; a wait queued ahead of its own release on a shared queue sits in front of it and never
 * ends.  sr_stream_wait_signal returns -6 when no release of `value` (or more) has been submitted for the signal yet. */
uint32_t    *sr_signal_alloc(sr_ctx *);
int          sr_signal_free(sr_ctx *, uint32_t *sig);
int          sr_stream_wait_signal(sr_ctx *, uint32_t *sig, uint32_t value);
int          sr_stream_write_signal(sr_ctx *, uint32_t *sig, uint32_t value);
int          sr_device_info(sr_ctx *, int *n_cu, int64_t *hbm_bytes, int *lds_per_cu, char *name, int name_len);
void        *sr_malloc(sr_ctx *, size_t bytes);     /* device memory                              */
int          sr_free(sr_ctx *, void *dev_ptr);
int          sr_memcpy_h2d(sr_ctx *, void *dev_dst, const void *host_src, size_t bytes);
int          sr_memcpy_d2h(sr_ctx *, void *host_dst, const void *dev_src, size_t bytes);
int          sr_memset(sr_ctx *, void *dev_dst, int value, size_t bytes);
/* Asynchronous copies on the context's stream (no synchronisation; the host buffer should be pinned: sr_host_alloc) and
 * page-locked host memory owned by the library.  A pipeline that keeps several batches in flight returns each batch's
 * results with these, on that batch's own stream -- no other runtime keeps per-stream state about the copies, so the
 * streams can be destroyed deterministically (sr_stream_destroy) when the pipeline closes. */
int          sr_memcpy_d2h_async(sr_ctx *, void *host_dst, const void *dev_src, size_t bytes);
int          sr_memcpy_h2d_async(sr_ctx *, void *dev_dst, const void *host_src, size_t bytes);
void        *sr_host_alloc(sr_ctx *, size_t bytes);              /* hipHostMalloc; NULL on failure */
int          sr_host_free(sr_ctx *, void *host_ptr);
int          sr_device_sync(sr_ctx *);                           /* every stream of the context's device */
/* HIP events on the context's stream (the stream the kernels are launched on). */
int          sr_timer_start(sr_ctx *);
int          sr_timer_stop_ms(sr_ctx *, float *elapsed_ms);     /* synchronises on the stop event */

/* ---- kernel 0: frame-major -> per-vector planes -------------------------------------------
 * Input is the layout the reference holds vectors in, (nframes, nvectors, 3) float32
 * (obtain_XHvecs, calculate-Ct-from-traj.py:64-86).  Output "SoA": soa[(v*3 + c)*Npad + n] for the
 * vector range [v0, v0+nV): the shard a GPU owns.  Npad >= N, Npad % 4 == 0. */
int sr_pack_soa_f32_dev(sr_ctx *, const float *vecs, int64_t N, int64_t Vtot, int64_t v0, int64_t nV,
                        float *soa, int64_t Npad);
/* Register tiles (128 frames x 32 vectors, one workgroup each) of the production form of kernel 0 for a shape, as a host function
 * that needs no context and no GPU: ceil(Npad / 128) * nV / 32 when the shape has whole 32-vector tiles and 16-byte rows (nV % 32 == 0,
 * Vtot * 3 and v0 * 3 multiples of 4, Npad a positive multiple of 4, 0 <= v0, v0 + nV <= Vtot), else 0: such a shape goes through the
 * LDS tile, as do arrays that are not 16-byte aligned. */
int64_t sr_pack_reg_tiles(int64_t Npad, int64_t Vtot, int64_t v0, int64_t nV);
/* The same with per-frame de-tumbling folded in: frame n is rotated by the unit
 * quaternion quat[n] = (w, x, y, z) -- rotate_vector_simd(v, q[:, None, :]), transforms3d_supplement.py:270-296, in
 * float64 -- before it is rounded into the float32 planes.  quat: DEVICE pointer, (N, 4) float64, already
 * normalised (vecnorm_NDarray).  With q = conj(q_orient(t)) from a PLUMED colvar-qorient file
 * (plumedcolvario.py:24-81) the planes hold body-frame vectors: lab-frame vectors + orientation trajectory in,
 * C(t) of the internal motion out, no superposition step (calculate-Ct-from-traj.py:466-467) needed. */
int sr_pack_soa_rot_f32_dev(sr_ctx *, const float *vecs, int64_t N, int64_t Vtot, int64_t v0, int64_t nV,
                            const double *quat, float *soa, int64_t Npad);

/* ---- kernel 1: Palmer-chunked P2 autocorrelation ------------------------------------------
 * Replaces calculate_Ct_Palmer (calculate-Ct-from-traj.py:200-238) after reformat_vecs_by_tau
 * (:245-275).  Chunk r covers frames [chunk_start[r], chunk_start[r]+F) of the packed planes
 * (chunk_start == NULL means r*F).  For delta = 1..L, L = F/2:
 *     p[r,v]      = (1/(F-delta)) * sum_j ( 1.5 (u[r,j,v].u[r,j+delta,v])^2 - 0.5 )
 *     Ct[d-1,v]   = mean_r p ;   dCt[d-1,v] = std_r(p, ddof=0) / (sqrt(R) - 1)
 * Ct, dCt are (L, nV) float64, row-major -- the reference's (nDeltas, nResidues).
 * mode 0 (production): the fastest formulation for the chunk length --
 *           1024 < F + L <= 8192: Wiener-Khinchin, (u.u')^2 = sum_c w_c a_c a_c' with a_c products of two components, one
 *           workgroup per (chunk, vector) with the whole transform in LDS.  4096 < F + L <= 8192 (cfg3 / cfg4): float32
 *           transforms of the five mean-removed traceless components, the mean terms restored in float64 (k_ct_rfft32:
 *           C(t) to 6e-8 on ordered vectors -- S2 near 0.9, the synthetic trajectories -- and to 1.6e-7 of C(0) on vectors that
 *           tumble, jump or sit on few sites, absolute where C(t) passes through zero: docs/EXPERIMENTS.md section 27; the class of
 *           the direct kernel and of the reference's own float32); shorter chunks: float64
 *           transforms (~1e-15).  sr_set_option("ct_fft", 2) selects float64 transforms everywhere, 0 disables the
 *           formulation;
 *           chunks beyond what the direct kernel can stage in LDS (about 13400 frames), up to sr_ct_max_frames_per_chunk() =
 *           262144 frames per chunk: the same decomposition with
 *           BLOCKED transforms (sr_ct_long.hip): blocks of 4096 samples, float32 forward transforms to a work area in device
 *           memory, cross-spectra per block offset and the inverse transforms in float64 (C(t) to 3.1e-8 on ordered vectors, to 1e-7
 *           of C(0) on mobile ones: section 27).  The series of a
 *           launch go in tiles whose spectra fit sr_set_option("ct_long_ws_mb", MiB) (default 256; results do not depend on it);
 *           sr_set_option("ct_long_min_frames", F0) (5462 .. 262144, default 16384) also gives them the chunks of F0 frames
 *           and more that the direct kernel could stage (F + L > 8192); by default the direct kernel keeps those.  Longer
 *           chunks are refused (-4);
 *           otherwise (short chunks, ct_fft = 0 or 1 beyond the transform lengths): direct shifted products, float32 dot products and short float32 partial sums folded into
 *           float64 (accurate to 3.5e-8 on ordered vectors, to 9e-8 of C(0) on mobile ones: the same section 27);
 * mode 1: direct shifted products, every product and sum in float64 (validation path).
 * The direct kernels stage a whole chunk in LDS (12 bytes per frame): mode 1 and ct_fft = 0 / 1 refuse chunks beyond about
 * 13400 frames (-4).
 * psum (optional, may be NULL): (nV, R, Lp) float64 raw sums  sum_j (u.u')^2, Lp = sr_ct_psum_stride(F). */
int64_t sr_ct_psum_stride(int64_t F);
/* Which formulation mode 0 / 1 runs for chunks of F frames under the options "ct_fft" and "ct_long_min_frames" when a workgroup may
 * have lds_limit bytes of LDS (sr_device_info: 163840 on gfx950) -- the dispatch of sr_ct_palmer_sums_f32_dev itself, as a host
 * function that needs no context and no GPU (like sr_ct_psum_stride).  With need = F + F/2, the length one transform must hold, and
 * "fits" = the direct kernel can stage the chunk in lds_limit: mode 1 is direct; in mode 0 chunks with need > 8192 are blocked
 * when ct_fft >= 2 and (F >= ct_long_min_frames or they do not fit); of the rest, ct_fft = 0, need <= 1024 and need > 8192 are direct,
 * ct_fft = 4 and (ct_fft = 3, need > 4096) float32 transforms, (ct_fft = 2, need > 4096) real-input float64 transforms, everything
 * else complex float64 transforms.  Whatever is left with the direct kernel and does not fit is refused (-4 from the entry points),
 * as are arguments outside their ranges. */
enum {
    SR_CT_REFUSED = 0,
    SR_CT_DIRECT = 1,      /* shifted products (k_ct_palmer) */
    SR_CT_FFT64 = 2,       /* complex float64 transforms (k_ct_fft) */
    SR_CT_RFFT64 = 3,      /* real-input float64 transforms (k_ct_rfft) */
    SR_CT_RFFT32 = 4,      /* real-input float32 transforms (k_ct_rfft32) */
    SR_CT_BLOCKED = 5      /* blocked float32 transforms through device memory (sr_ct_long.hip) */
};
int sr_ct_formulation(int ct_fft, int64_t ct_long_min_frames, int mode, int64_t F, int64_t lds_limit);
int64_t sr_ct_max_frames_per_chunk(sr_ctx *);
/* the two halves of sr_ct_palmer_f32_dev as separate launches: raw sums per (vector, chunk, lag) into caller memory
 * (psum: (nV, R, Lp) float64, required here), then mean / std over the chunks (calculate-Ct-from-traj.py:226-228).
 * A pipeline with several batches in flight gives every batch its own psum; timing the first call alone gives the
 * duration of the dominant kernel. */
int sr_ct_palmer_sums_f32_dev(sr_ctx *, const float *soa, int64_t Npad, int64_t R, int64_t F, int64_t nV,
                              const int64_t *chunk_start_host, int mode, double *psum);
/* sr_ct_palmer_sums_f32_dev, and kernel 0 of the NEXT batch with it: next_vecs (next_N, next_Vtot, 3), columns [next_v0, next_v0 +
 * next_nV), are packed into next_soa (next_Npad floats per plane) exactly as sr_pack_soa_f32_dev packs them -- an independent job,
 * validated like that call; next_soa must overlap neither soa nor psum (-3).  When sr_ct_pack_fused() admits the pair, ONE launch does
 * both: every workgroup of the C(t) kernel moves one or two register tiles of the pack in front of its own work, so the pack needs no
 * wave slot beside the C(t) grids and its planes are complete when the launch is.  Otherwise kernel 0 is launched in front of the
 * C(t) kernel on the same stream.  Planes and sums are the same bits either way, and what is refused queues nothing. */
int sr_ct_palmer_sums_pack_f32_dev(sr_ctx *, const float *soa, int64_t Npad, int64_t R, int64_t F, int64_t nV,
                                   const int64_t *chunk_start_host, int mode, double *psum,
                                   const float *next_vecs, int64_t next_N, int64_t next_Vtot, int64_t next_v0, int64_t next_nV,
                                   float *next_soa, int64_t next_Npad);
/* What that call would do with the same arguments, without queueing anything: 1 = one launch carries the pack, 0 = kernel 0 in front of
 * the C(t) kernel, negative = the refusal.  (A pipeline that keeps its pack on another stream unless it is carried asks first.) */
int sr_ct_palmer_sums_pack_plan(sr_ctx *, const float *soa, int64_t Npad, int64_t R, int64_t F, int64_t nV,
                                const int64_t *chunk_start_host, int mode, const double *psum,
                                const float *next_vecs, int64_t next_N, int64_t next_Vtot, int64_t next_v0, int64_t next_nV,
                                const float *next_soa, int64_t next_Npad);
/* The rule of that choice, as a host function (no context, no GPU): 1 when the launch carries the pack.  formulation: what
 * sr_ct_formulation() gives for the C(t) job; F its chunk length; series = R * nV, its workgroups; tiles = sr_pack_reg_tiles() of the
 * pack job; aligned: the planes read are 8-byte aligned with even Npad and chunk starts (the kernel without frame masks), and
 * next_vecs, next_soa are 16-byte aligned.  Carried: float32 transforms at F = 4096 (cfg3 / cfg4: the one instantiation built), aligned,
 * and 1 <= tiles <= 2 * series. */
int sr_ct_pack_fused(int formulation, int64_t F, int64_t series, int64_t tiles, int aligned);
int sr_ct_finalize_f64_dev(sr_ctx *, const double *psum, int64_t R, int64_t F, int64_t nV, double *Ct, double *dCt);
/* the same launch also leaves the transposed copies CtT, dCtT (nV, L) the fits read (fitting_Ct_functions.py:149 works
 * per residue); both NULL = not wanted. */
int sr_ct_finalize_t_f64_dev(sr_ctx *, const double *psum, int64_t R, int64_t F, int64_t nV, double *Ct, double *dCt,
                             double *CtT, double *dCtT);
int sr_ct_palmer_f32_dev(sr_ctx *, const float *soa, int64_t Npad, int64_t R, int64_t F, int64_t nV,
                         const int64_t *chunk_start_host, int mode,
                         double *psum_ws, double *Ct, double *dCt);
/* host-buffer form: vecs is (N, Vtot, 3) float32 on the host, N >= R*F when chunk_start is NULL. */
int sr_ct_palmer_f32(sr_ctx *, const float *vecs, int64_t N, int64_t Vtot, int64_t v0, int64_t nV,
                     int64_t R, int64_t F, const int64_t *chunk_start_host, int mode,
                     double *Ct, double *dCt);

/* ---- kernel 2: quaternion rotation + Lambert-cylindrical histogram + mean vector + S2 ------
 * Replaces rotate_vector_simd (transforms3d_supplement.py:270-296), xyz_to_rtp
 * (general_maths.py:118-158), the per-bond np.histogramdd loop (calculate-Ct-from-traj.py:600-626),
 * the mean vector (:579-583) and calculate_S2_by_outerProduct (:96-145) in one pass over the planes.
 *   q           : 4 doubles (w,x,y,z), normalised inside like the reference; NULL = no rotation;
 *   edges_phi   : nphi+1 doubles, edges_cos: ncos+1 doubles -- numpy.linspace(-pi, pi, nphi+1) and numpy.linspace(-1, 1, ncos+1),
 *                 the edges np.histogramdd builds for range=((-pi, pi), (-1, 1)).  The kernel places most samples by arithmetic on
 *                 equal bins, so the call returns -3 unless each array is strictly increasing, starts and ends at those values to
 *                 1e-12 and has every edge within 1e-9 bin widths of its uniform position; binning is
 *                 numpy's: searchsorted(edges, x, 'right')-1, last edge inclusive, outside/NaN dropped;
 *   hist        : (nV, nphi, ncos) float64 counts (the dtype the reference stores);
 *   vecsum      : (nV, 3) float64 sum over the first N frames of the rotated vectors (may be NULL);
 *   outer       : (nBlocks, nV, 6) float64 sums of xx,yy,zz,xy,xz,yz per block of block_len frames
 *                 (may be NULL; nBlocks = N_used / block_len). */
int sr_rotate_hist_f32_dev(sr_ctx *, const float *soa, int64_t Npad, int64_t N, int64_t nV,
                           const double *q_host, const double *edges_phi_host, int nphi,
                           const double *edges_cos_host, int ncos,
                           double *hist, double *vecsum, double *outer, int64_t block_len);
int sr_rotate_hist_f32(sr_ctx *, const float *vecs, int64_t N, int64_t Vtot, int64_t v0, int64_t nV,
                       const double *q, const double *edges_phi, int nphi, const double *edges_cos, int ncos,
                       double *hist, double *vecsum, double *outer, int64_t block_len);
/* How kernel 2 cuts the N frames of a call with nV vectors into ranges -- the computation of sr_rotate_hist_f32_dev itself, as a host
 * function that needs no context and no GPU (like sr_ct_formulation).  Fb = block_len when 0 < block_len <= N, else N; nB = N / Fb
 * full S2 blocks; every block is cut into m ranges of sub frames (sub % 4 == 0, sub <= 8192, the last one shorter); the frames behind
 * the last full block form further ranges of sub frames; nranges counts all of them.  Range rid < nB * m starts at frame
 * (rid / m) * Fb + (rid % m) * sub, a later one at nB * Fb + (rid - nB * m) * sub; ranges 4 k .. 4 k + 3 share a workgroup.  Any
 * output pointer may be NULL.  Returns -3 for N < 1 or nV < 1. */
int sr_vechist_plan(int64_t N, int64_t nV, int64_t block_len, int64_t *Fb, int *nB, int *m, int64_t *sub, int *nranges);
/* rotated vectors themselves, float64 (N, nV, 3) like the reference returns (for --vecDist output). */
int sr_rotate_vectors_f32(sr_ctx *, const float *vecs, int64_t N, int64_t Vtot, int64_t v0, int64_t nV,
                          const double *q, double *out);
/* one quaternion per frame: quat (N, 4) float64 host array, already normalised; out (N, nV, 3) float64. */
int sr_rotate_vectors_perframe_f32(sr_ctx *, const float *vecs, int64_t N, int64_t Vtot, int64_t v0, int64_t nV,
                                   const double *quat, double *out);

/* ---- resident bond vectors: upload once, pack once (a rank owns a vector range) --------------
 * The reference keeps vecXH / vecXHfit in host arrays (calculate-Ct-from-traj.py:464-498) and reads them for C(t) of the
 * lab-frame vectors (:527), C(t) of the fitted ones (:530) and the rotation + histogram + mean vector + S2 pass (:541-646).
 * An sr_vectors object holds ONE rank's columns [v0, v0 + nV) of such an array on the device:
 *   sr_vectors_create        nV vectors, room for capacity_frames frames (grows when more are appended); NULL on failure
 *   sr_vectors_append_f32    n more frames from a HOST array (n, Vtot, 3): only the bytes of columns [v0, v0 + nV) cross
 *                            PCIe (row pitch 12 Vtot, width 12 nV), through two pinned staging buffers; synchronous with
 *                            respect to the host array, asynchronous on the device.  A PAGE-LOCKED source (sr_host_alloc,
 *                            hipHostMalloc / hipHostRegister) is read by the copy engine directly -- one asynchronous (2-D)
 *                            copy, no staging pass; the caller then keeps it unchanged until the stream has passed the call
 *   sr_vectors_frame_major_dev  device address of the (frames, nV, 3) array held (NULL on failure); work queued on the
 *                            context's stream behind this call sees every appended frame (the feed of a device pipeline)
 *   sr_vectors_append_dev    n more frames from a DEVICE array (n, nV, 3) (e.g. an output of sr_xh_vectors_f32_dev)
 *   sr_vectors_append_xyz_f32  n more frames straight from HOST coordinates: obtain_XHvecs (+ centre / superpose) of
 *                            sr_xh_vectors_f32_dev for the bonds idxX[i] -> idxH[i], i < nV (the rank's slice of the
 *                            selections), written into `lab` and / or `fit` (either may be NULL) -- the streaming form of
 *                            the reference's --split loop (:426-453): the host never holds more than one chunk
 *   sr_vectors_truncate      keep the first n_frames frames (reformat_vecs_by_tau drops the tail of every file that does not fill
 *                            a block of memory time, calculate-Ct-from-traj.py:259-272: a streamed file is cut when it ends)
 *   sr_vectors_download_f32  frames [f0, f0 + n) back to the host as (n, nV, 3) (the --vecDist outputs need them)
 *   sr_vectors_ct_f32        kernel 0 (once per object) + kernel 1: as sr_ct_palmer_f32, Ct / dCt (F/2, nV) on the host
 *   sr_vectors_hist_f32      kernel 0 (once per object) + kernel 2 over the first N_hist frames (<= 0: all): as
 *                            sr_rotate_hist_f32
 * Stream ordering: an append leaves its copies in flight on the context's current stream and records an event behind
 * them; every consumer (ct, ct_sums, hist, download, frame_major_dev) AND every further append first makes ITS current stream
 * wait for that event, so sr_set_stream between an append and the next use or the next append loses no ordering (appends on
 * different streams chain; the growth copy of a full object runs behind the frames it copies).  chunk_start_host tables are range-checked against the frames held.
 * sr_counter(ctx, "h2d_vector_bytes" | "vector_uploads"): bytes and calls of sr_vectors_append_f32 since sr_create (the
 * host-pointer entry points sr_ct_palmer_f32 / sr_rotate_hist_f32 go through it too). */
typedef struct sr_vectors sr_vectors;
sr_vectors *sr_vectors_create(sr_ctx *, int64_t nV, int64_t capacity_frames);
void        sr_vectors_destroy(sr_ctx *, sr_vectors *);
int64_t     sr_vectors_frames(const sr_vectors *);
const float *sr_vectors_frame_major_dev(sr_ctx *, sr_vectors *);
int sr_vectors_truncate(sr_ctx *, sr_vectors *, int64_t n_frames);
int sr_vectors_append_f32(sr_ctx *, sr_vectors *, const float *vecs_host, int64_t n, int64_t Vtot, int64_t v0);
int sr_vectors_append_dev(sr_ctx *, sr_vectors *, const float *vecs_dev, int64_t n);
int sr_vectors_append_xyz_f32(sr_ctx *, sr_vectors *lab, sr_vectors *fit, const float *xyz_host, int64_t nFrames, int64_t nAtoms,
                              const int32_t *idxX, const int32_t *idxH, int nV, const int32_t *fit_idx, int nFit,
                              const float *ref_xyz);
int sr_vectors_download_f32(sr_ctx *, const sr_vectors *, int64_t f0, int64_t n, float *out_host);
int sr_vectors_ct_f32(sr_ctx *, sr_vectors *, int64_t R, int64_t F, const int64_t *chunk_start_host, int mode,
                      double *Ct, double *dCt);
/* Fewer vectors than GPUs: ranks own ranges of CHUNKS instead (last paragraph).  A rank computes the
 * raw sums S[v][r][d-1] = sum_j (u_j . u_{j+d})^2 of ITS chunks, (nV, R, L) float64 on the host; the gathered (nV, R_total, L)
 * array goes through the same mean / std kernel that finishes a single-process run (calculate-Ct-from-traj.py:226-228: mean
 * and two-pass std over the replicates need every replicate's value, not running sums). */
int sr_vectors_ct_sums_f32(sr_ctx *, sr_vectors *, int64_t R, int64_t F, const int64_t *chunk_start_host, int mode, double *sums);
int sr_ct_finalize_sums_f64(sr_ctx *, const double *sums_host, int64_t R, int64_t F, int64_t nV, double *Ct, double *dCt);
int sr_vectors_hist_f32(sr_ctx *, sr_vectors *, int64_t N_hist, const double *q, const double *edges_phi, int nphi,
                        const double *edges_cos, int ncos, double *hist, double *vecsum, double *outer, int64_t block_len);
int sr_counter(sr_ctx *, const char *name, uint64_t *value);

/* ---- iRED: equal-time P2 cross-correlation matrix of the bond vectors ----------------------------------------------------
 * The isotropic reorientational eigenmode dynamics analysis (Prompers & Brueschweiler, J. Am. Chem. Soc. 124, 4522 (2002);
 * its windowed form for long trajectories: Gu, Li & Brueschweiler, J. Chem. Theory Comput. 10, 2599 (2014)) that the reference
 * announces in calculate_S2_by_iRED / calculate_S2_by_wiRED (calculate-S2.py:158-191) and leaves as stubs that stop after the
 * window length.  Built to the publications.  For window w = frames [win_start[w], win_start[w] + win_len[w]) of the planes:
 *     M[w][i][j] = (1 / F_w) sum_t ( 1.5 (u_i(t) . u_j(t))^2 - 0.5 ),   F_w = win_len[w],  i, j < nV
 * (nV, nV) float64 per window, exactly symmetric.  The literal definition: no unit-length assumption, a (0,0,0) vector (what
 * vecnorm_NDarray makes of 0/0) contributes -0.5.  The eigen-decomposition and S2 = 1 - sum_{m > G} lambda_m |m>_i^2 are host work
 * (spinrelax_amd/ired.py).
 * (u_i.u_j)^2 = sum_{a<=b} w_ab (u_ia u_ib)(u_ja u_jb), w = 1, 1, 1, 2, 2, 2: a symmetric rank-k update over K = 6 F_w whose
 * operands, products of two float32 values, are exact in float64 (the 2 is put on one side).  k_ired_matrix accumulates the 64 x 64
 * tiles with tile row <= tile column on the float64 matrix pipe (v_mfma_f64_16x16x4_f64), operands formed in registers from float32
 * x, y, z staged in LDS; a window's frames are shared by S workgroups per tile pair, whose partial tiles go to a context work area;
 * k_ired_finish adds the S partials in fixed order, applies 1.5 / F_w and -0.5 and writes both triangles.  No atomics: equal input
 * and equal S give bit-equal M.  S = "ired_ksplit" when set, else min(64, max(1, Fmax / 256), ceil(1024 / (W T (T + 1) / 2))) with
 * T = ceil(nV / 64) and Fmax the longest window: about four workgroups per CU, at least 256 frames each.
 * The window tables are HOST arrays of W entries, range-checked (0 <= start, 1 <= len, start + len <= Npad; the sr_vectors form:
 * against the frames held) before anything is queued and consumed on return.  nV < 1, W < 1 and a window shorter than one frame
 * are refused (-3).  M_dev: DEVICE, (W, nV, nV) float64. */
int sr_ired_matrix_f32_dev(sr_ctx *, const float *soa, int64_t Npad, int64_t nV, const int64_t *win_start_host,
                           const int64_t *win_len_host, int W, double *M_dev);
/* kernel 0 (once per object; the planes that sr_vectors_ct_f32 / sr_vectors_hist_f32 left are reused) + the two kernels above;
 * M_host: (W, nV, nV) float64 on the host.  Blocks until M is there. */
int sr_vectors_ired_f32(sr_ctx *, sr_vectors *, const int64_t *win_start_host, const int64_t *win_len_host, int W, double *M_host);

/* ---- iRED: time-correlation functions of the modes -------------------------------------------------------------------------
 * The dynamics half of the analysis (same publications).  For window w and row m of its coefficient matrix coef[w] (K rows of nV
 * weights e_mi, float64; the production caller passes the eigenvectors of M[w] as rows, the kernels take any matrix), with c over
 * (xx, yy, zz, xy, xz, yz) and w_c = 1, 1, 1, 2, 2, 2:
 *     A_mc(t) = sum_i e_mi u_ia(t) u_ib(t)
 *     C_m(k)  = 1.5 / (F_w - k) sum_{tau = 0}^{F_w - k - 1} sum_c w_c A_mc(tau) A_mc(tau + k) - 0.5 sigma_m^2,   sigma_m = sum_i e_mi
 *             = sum_ij e_mi e_mj < 1.5 (u_i(tau) . u_j(tau + k))^2 - 0.5 >_tau,      k = 0 .. n_lags - 1
 * No unit-length assumption, like M; with eigenvectors as rows C_m(0) = lambda_m.
 * k_ired_project forms the amplitudes as a GEMM over the vectors on the float64 matrix pipe (v_mfma_f64_16x16x4_f64; the operands
 * u_a u_b are formed in registers from float32 x, y, z and are exact, the only rounding is the accumulation) into a context work
 * area, 48 K F_w bytes per window; k_ired_mode_ct, one workgroup per (window, mode), takes the six amplitude series through the
 * in-LDS float64 transforms of kernel 1's k_ct_fft (three packed pairs, weighted power spectrum, one transform back) with
 * M = 2048 / 4096 / 6144 / 8192 points, the smallest M >= F_w + n_lags - 1.  The windows of a call go in batches whose amplitudes fit
 * "ired_ws_mb".  No atomics and no split of a reduction: equal input gives bit-equal output, whatever the batches.
 * The window tables are HOST arrays, range-checked like sr_ired_matrix_f32_dev's before anything is queued.  Refused with -3:
 * K < 1, n_lags < 1, a window with n_lags > F_w; with -4: a window with F_w + n_lags - 1 > 8192 (blocked transforms for longer
 * windows do not exist yet).  coef_dev: DEVICE, (W, K, nV) float64; Cm_dev: DEVICE, (W, K, n_lags) float64.  Asynchronous. */
int sr_ired_mode_ct_f32_dev(sr_ctx *, const float *soa, int64_t Npad, int64_t nV, const int64_t *win_start_host,
                            const int64_t *win_len_host, int W, const double *coef_dev, int K, int n_lags, double *Cm_dev);
/* the same of resident vectors, coefficient matrices and result on the HOST.  Blocks until Cm is there. */
int sr_vectors_ired_mode_ct_f32(sr_ctx *, sr_vectors *, const int64_t *win_start_host, const int64_t *win_len_host, int W,
                                const double *coef_host, int K, int n_lags, double *Cm_host);

/* ---- all-pairs dipolar map: <r^-6>, <r^-3> and the order tensor of every pair of a set of spins (sr_noe.hip; beyond the reference) ----
 * The screening step in front of the dipolar correlation functions (Brueschweiler et al., JACS 114, 2289 (1992); Peter, Daura &
 * van Gunsteren, J. Biomol. NMR 20, 297 (2001)).  For the P atoms index[0 .. P) of coordinates xyz (nFrames, nAtoms, 3) float32, per
 * frame block b = frames [block_start[b], block_start[b] + block_len[b]) and per pair i < j (positions in `index`), with
 * d = x_index[j] - x_index[i], r = |d| and d' = R(quat[t]) d:
 *     sums[b][k(i, j)][0]      = sum_t r^-6
 *     sums[b][k(i, j)][1 .. 6] = sum_t d'_a d'_b r^-5   for ab = xx, yy, zz, xy, xz, yz        (xx + yy + zz = sum_t r^-3)
 * k(i, j) = i (2 P - i - 1) / 2 + (j - i - 1): row-major over i < j.  The averages, effective distances and order parameters are host
 * work (spinrelax_amd/noe.py).  d is the difference of the raw float32 coordinates, taken first and in the lab frame; r and its
 * powers come from it, and only the tensor sees the rotation (applied to d, never to the coordinates).
 *   mode 0: float32 per pair and frame: d, r^2 = fma(dz, dz, fma(dy, dy, dx dx)), v_rsq_f32, r^-3 = (ri ri) ri, r^-5 = r^-3 (ri ri),
 *           r^-6 = r^-3 r^-3, R rounded to float32; float32 partial sums of at most 8 frames, then float64.
 *   mode 1: float64 throughout (the on-device check).
 * k_noe_pairs: one workgroup of 256 threads per (block, frame split, tile pair ti <= tj) of T x T atoms, T = sr_noe_tile(), 2 x 2
 * pairs per thread; the two tiles' coordinates of sr_noe_frame_batch() frames are gathered into LDS, the frame's rotation matrix is
 * formed once per workgroup.  Of a diagonal tile only i < j is kept.  k_noe_finish adds the S partial tiles in the order s = 0 .. S-1.
 * No atomics: equal input gives bit-equal sums.  S is a function of the shape alone: min(256, max(1, Fmax / 128),
 * ceil(4096 / (B tile pairs))).  With S > 1 the partial tiles are a work area of S times 1.03 to 1.13 times the bytes of sums (whole
 * tiles); with S = 1 -- every map of 4096 or more tile pairs, P > 2850 or so in one block -- k_noe_pairs writes sums itself and the call
 * needs no memory beside its result.
 *   index_host (P) distinct atom indices, block tables (B): HOST arrays, checked before anything is queued and consumed on return;
 *   quat: DEVICE (nFrames, 4) float64 unit quaternions (w, x, y, z) as sr_xh_vectors_f32_dev writes them, NULL = identity;
 *   sums: DEVICE (B, P (P - 1) / 2, 7) float64.  Asynchronous on the context's stream.
 * Refused with -3, before anything is queued: P < 2, an index out of range or duplicated, B < 1, a block shorter than one frame or
 * outside the frames, a mode other than 0 or 1, and a result of B P (P - 1) / 2 * 56 bytes (plus the partial tiles) beyond the
 * device's memory.  A pair that coincides in some frame gives a non-finite sum (the caller's to report). */
int sr_noe_pairs_f32_dev(sr_ctx *, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index_host, int64_t P,
                         const double *quat, const int64_t *block_start_host, const int64_t *block_len_host, int B, int mode,
                         double *sums);
/* the same with xyz, quat (may be NULL) and sums on the HOST.  Blocks until sums is there. */
int sr_noe_pairs_f32(sr_ctx *, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const double *quat,
                     const int64_t *block_start, const int64_t *block_len, int B, int mode, double *sums);
/* What the two calls above refuse with -3, with their message, and nothing else: all host work, nothing allocated or queued.  For a
 * caller that has to allocate sums itself and wants to hear of a map beyond the device's memory first. */
int sr_noe_pairs_check(sr_ctx *, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const int64_t *block_start,
                       const int64_t *block_len, int B, int mode);
int sr_noe_tile(void);          /* T: atoms per tile side (tests aim at tile edges) */
int sr_noe_frame_batch(void);   /* frames per LDS stage of k_noe_pairs */

/* ---- the all-pairs dipolar map at a few chosen lags (sr_noe.hip; beyond the reference) ----------------------------------------
 * For the same atoms, blocks and pair order, and K lags k = lags[0] < lags[1] < ...:
 *     G[b][q][k(i, j)] = sum over the origins t of block b with t + k inside the block of
 *                        [1.5 (d'(t) . d'(t + k))^2 / (r(t)^2 r(t + k)^2) - 0.5] r(t)^-3 r(t + k)^-3,      d'(t) = R(quat[t]) d(t)
 * the unnormalised dipolar correlation function of every pair at lag k; G at lag 0 is the map's r^-6 sum.  C_dd(k) and the per-pair
 * internal correlation time are host work (spinrelax_amd/noe.py).
 *   mode 0: float32 per pair, frame and lag: d, e the differences at t and t + k; r2, s2 by the map's two-fma chain; v_rsq_f32 of
 *           both; d', e' by three fmas per component, R rounded to float32; c = fma(d'z, e'z, fma(d'y, e'y, d'x e'x)); g = ri si;
 *           x = c g; g3 = (g g) g; p = fma(1.5 x, x, -0.5); term = p g3; float32 partial sums of at most 8 origins, then float64.
 *   mode 1: the same sequence in float64 with 1 / sqrt.
 * k_noe_lagged: one workgroup per (block, lag, frame split, tile pair), tiles and threads as in k_noe_pairs, two windows of
 * sr_noe_frame_batch() frames in LDS (the origins and the frames one lag later).  A frame split owns a range of origins, runs of
 * ceil((n_b - k) / S); k_noe_finish adds the S partial tiles in the order s = 0 .. S-1.  No atomics: equal input gives
 * bit-equal G.  S = sr_noe_lagged_splits(P, longest block, B) is the map's split count and does not depend on the lags: a lag has the
 * same bits alone and in any list.  With S > 1 the partial tiles are a work area of about S times the bytes of G.
 *   lags_host (K) int32: HOST array, like the index and the block tables; G: DEVICE (B, K, P (P - 1) / 2) float64.  Asynchronous on
 *   the context's stream.
 * Refused with -3, before anything is queued: everything sr_noe_pairs_check refuses; K < 1 or K > 64; a negative lag; lags that are
 * not strictly increasing; a largest lag >= the shortest block (every (block, lag) has at least one term); G plus the partial tiles
 * beyond the device's memory; B K S tile pairs >= 2^31 workgroups. */
int sr_noe_lagged_f32_dev(sr_ctx *, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index_host, int64_t P,
                          const double *quat, const int64_t *block_start_host, const int64_t *block_len_host, int B,
                          const int32_t *lags_host, int K, int mode, double *G);
/* the same with xyz, quat (may be NULL) and G on the HOST.  Blocks until G is there. */
int sr_noe_lagged_f32(sr_ctx *, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const double *quat,
                      const int64_t *block_start, const int64_t *block_len, int B, const int32_t *lags, int K, int mode, double *G);
/* What the two calls above refuse with -3, with their message, and nothing else: all host work, nothing allocated or queued. */
int sr_noe_lagged_check(sr_ctx *, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const int64_t *block_start,
                        const int64_t *block_len, int B, const int32_t *lags, int K, int mode);
int sr_noe_lagged_splits(int64_t P, int64_t longest_block, int B);   /* S of such a call (tests aim at S > 1); 0 for a bad shape */

/* ---- the lagged map split into the five tumbling modes of an anisotropic diffusion tensor (sr_noe.hip; beyond the reference) ----
 * For the same atoms, blocks, lags and pair order as sr_noe_lagged_*, six sums per (block, lag, pair).  With F = R(frame_quat), the
 * constant rotation into the principal-axis frame of the diffusion tensor, d"(t) = F R(quat[t]) d(t), u = d"(t) / r(t),
 * v = d"(t + k) / r(t + k), w = r(t)^-3 r(t + k)^-3, qz(u) = u_z^2 - 1/3 and dl(u) = u_x^2 - u_y^2:
 *     H[b][q][k(i, j)][0 .. 5] = sum over the origins t of block b with t + k inside the block of
 *         w qz(u) qz(v),   w dl(u) dl(v),   w [qz(u) dl(v) + dl(u) qz(v)] / 2,   w u_y u_z v_y v_z,   w u_x u_z v_x v_z,   w u_x u_y v_x v_y
 * They do not depend on the tensor: one H serves any D.  2.25 H0 + 0.75 H1 + 3 (H3 + H4 + H5) is G of sr_noe_lagged_* whatever the
 * frame; the amplitudes of the five modes are host work (spinrelax_amd/noe.py: mode_amplitudes).
 *   mode 0: float32 per pair, frame and lag: d, e, r2, s2, ri, si, d', e' as in k_noe_lagged with the matrix F R(quat[t]), formed in
 *           float64 and rounded to float32; u_a = d'_a ri, v_a = e'_a si; a0 = fma(uz, uz, -1/3), a1 = fma(ux, ux, -(uy uy)), b0, b1
 *           of v likewise; g = ri si; g3 = (g g) g; the six terms (a0 b0) g3, (a1 b1) g3, (0.5 fma(a0, b1, a1 b0)) g3,
 *           ((uy uz) (vy vz)) g3, ((ux uz) (vx vz)) g3, ((ux uy) (vx vy)) g3; float32 partial sums of at most 8 origins, then float64.
 *   mode 1: the same sequence in float64 with 1 / sqrt.
 * k_noe_modes and k_noe_finish: the workgroups, tiles, windows, origin ranges and the split count S = sr_noe_lagged_splits(...)
 * of k_noe_lagged; the partial tiles are added in the order s = 0 .. S-1.  No atomics: equal input gives bit-equal H, and a lag has
 * the same bits alone and in any list.  With S > 1 the partial tiles are a work area of about S times the bytes of H.
 *   quat: DEVICE (nFrames, 4) float64 or NULL (R(quat[t]) = 1); frame_quat_host: HOST (4) float64 (w, x, y, z), a unit quaternion
 *   (normalised again in float64 before use), or NULL (F = 1); with both NULL no rotation is applied at all.
 *   H: DEVICE (B, K, P (P - 1) / 2, 6) float64.  Asynchronous on the context's stream.
 * Refused with -3, before anything is queued: everything sr_noe_lagged_check refuses, the byte counts taken six times; a frame
 * quaternion that is not finite or whose squared norm is farther than 1e-6 from 1. */
int sr_noe_modes_f32_dev(sr_ctx *, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index_host, int64_t P,
                         const double *quat, const double *frame_quat_host, const int64_t *block_start_host,
                         const int64_t *block_len_host, int B, const int32_t *lags_host, int K, int mode, double *H);
/* the same with xyz, quat (may be NULL) and H on the HOST.  Blocks until H is there. */
int sr_noe_modes_f32(sr_ctx *, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const double *quat,
                     const double *frame_quat, const int64_t *block_start, const int64_t *block_len, int B, const int32_t *lags, int K,
                     int mode, double *H);
/* What the two calls above refuse with -3, with their message, and nothing else: all host work, nothing allocated or queued. */
int sr_noe_modes_check(sr_ctx *, int64_t nFrames, int64_t nAtoms, const int32_t *index, int64_t P, const int64_t *block_start,
                       const int64_t *block_len, int B, const int32_t *lags, int K, const double *frame_quat, int mode);

/* ---- NOESY intensities from the dipolar map: the full relaxation matrix (sr_noesy.hip; beyond the reference) -------------------------
 * Macura & Ernst, Mol. Phys. 41, 95 (1980); Keepers & James, J. Magn. Reson. 57, 404 (1984); the model-free rates from <r^-6> and S2:
 * Brueschweiler et al., JACS 114, 2289 (1992).  Isotropic tumbling, one kind of spin.  With A6 and S2 (P (P - 1) / 2 each) in the pair
 * order of the map, k(i, j) = i (2 P - i - 1) / 2 + (j - i - 1):
 *     J(w)     = S2 tau_c / (1 + w^2 tau_c^2) + (1 - S2) t' / (1 + w^2 t'^2),      1 / t' = 1 / tau_c + 1 / tau_e
 *     R_ij     = sigma_ij = prefactor A6 [6 J(2 omega_H) - J(0)]                   (i != j; R_ji the same bits)
 *     R_ii     = sum_j prefactor A6 [J(0) + 3 J(omega_H) + 6 J(2 omega_H)] + leak_i
 * prefactor = 0.1 (mu0 / 4 pi)^2 hbar^2 gamma_H^4 / u^6, u = metres per unit of the coordinates that A6 was taken in.  tau_e_pair
 * (one per pair) and leak_spin (one per spin) may be NULL: the scalars tau_e and leak then hold for all, and are ignored otherwise.
 * S2 is clipped to [0, 1].  k_noesy_rates: one workgroup per row, the row sum in a fixed order, no atomics.
 *   A6, S2, tau_e, leak: HOST arrays, checked before anything is queued and consumed on return; R_dev: DEVICE (P, P) float64.
 * Refused with -3, before anything is queued: P < 2 or P > 32768, an A6 that is not finite and > 0, an S2 outside [-1e-6, 1 + 1e-6],
 * tau_c <= 0, a tau_e <= 0, a negative leak, a prefactor <= 0, a negative omega_H, anything not finite. */
int sr_noesy_rates_f64_dev(sr_ctx *, const double *A6_host, const double *S2_host, const double *tau_e_host, const double *leak_host,
                           int64_t P, double omega_H, double tau_c, double tau_e, double leak, double prefactor, double *R_dev);
/* the same with R on the HOST.  Blocks until R is there. */
int sr_noesy_rates_f64(sr_ctx *, const double *A6, const double *S2, const double *tau_e_pair, const double *leak_spin, int64_t P,
                       double omega_H, double tau_c, double tau_e, double leak, double prefactor, double *R);
/* The same matrix under anisotropic tumbling: the diffusion tensor's five rates E[0 .. 4] (1 / s, the order of
 * _hostmath.D_coefficients_ellipsoid) and per pair the mode amplitudes a[k][m] at lag 0 and their plateaus c[k][m] (units of A6:
 * sum_m a = A6, sum_m c = S2 A6; spinrelax_amd/noe.py: mode_amplitudes, mode_plateau), g(x, y) = x / (x^2 + y^2):
 *     J(w)     = sum_m [ c_m g(E_m, w) + max(a_m - c_m, 0) g(E_m + 1 / tau_e, w) ]
 *     R_ij     = prefactor [6 J(2 omega_H) - J(0)],      R_ii = sum_j prefactor [J(0) + 3 J(omega_H) + 6 J(2 omega_H)] + leak_i
 * With E_m = 1 / tau_c for all m this is the formula above.  tau_e: tau_e_mode (one per pair and mode), else tau_e_pair (one per
 * pair), else the scalar.  k_noesy_rates_modes: one workgroup per row, the row sum in a fixed order, R_ij and R_ji the same bits.
 *   a, c (P (P - 1) / 2, 5), E (5), tau_e_pair, tau_e_mode (P (P - 1) / 2, 5), leak: HOST arrays, checked before anything is queued
 *   and consumed on return; R_dev: DEVICE (P, P) float64.
 * Refused with -3, before anything is queued: P < 2 or P > 32768, tables beyond the device's memory, a negative a or c,
 * c_m > a_m (1 + 1e-6) where a_m > 0 (c_m > 0 where a_m = 0), E_m <= 0, a tau_e <= 0, a negative leak, a prefactor <= 0, a negative
 * omega_H, anything not finite. */
int sr_noesy_rates_modes_f64_dev(sr_ctx *, const double *a_host, const double *c_host, const double *E_host, const double *tau_e_pair_host,
                                 const double *tau_e_mode_host, const double *leak_host, int64_t P, double omega_H, double tau_e,
                                 double leak, double prefactor, double *R_dev);
/* the same with R on the HOST.  Blocks until R is there. */
int sr_noesy_rates_modes_f64(sr_ctx *, const double *a, const double *c, const double *E, const double *tau_e_pair,
                             const double *tau_e_mode, const double *leak_spin, int64_t P, double omega_H, double tau_e, double leak,
                             double prefactor, double *R);
/* C = alpha A B + beta I for symmetric (P, P) float64 DEVICE matrices A and B that commute; C may be A or B.  Only the 64 x 64 tiles
 * with tile row <= tile column are computed (k_symm_mul: v_mfma_f64_16x16x4_f64, both operands read as rows, k split over S
 * workgroups, S a function of P alone) and k_symm_mul_finish writes C[i][j] and C[j][i] from one value: C == C^T bit for bit, equal
 * input gives equal bits.  For symmetric input that does not commute the result is DEFINED as those tiles of alpha A B + beta I (of a
 * diagonal tile the entries i <= j), mirrored below.  1 <= P <= 32768.  Asynchronous on the context's stream. */
int sr_symm_mul_f64_dev(sr_ctx *, const double *A, const double *B, int64_t P, double alpha, double beta, double *C);
/* out[k] = exp(-R tau[k]), k < n_tau, for a symmetric DEVICE matrix R (P, P) float64 and HOST mixing times tau, into the DEVICE array
 * out (n_tau, P, P) float64, by scaling and squaring: s and the number of products as sr_symm_expm_plan gives them for |R|_1 (row
 * sums on the device, their maximum on the host), Y = -R tau / 2^s, the Taylor polynomial of degree 12 by Horner, s squarings, every
 * product by sr_symm_mul_f64_dev's kernels.  Each mixing time is computed from R on its own (equal bits alone and in a list).
 * Refused with -3: P outside 1 .. 32768, n_tau < 1, a tau that is not finite or negative, results plus work area beyond the device's
 * memory or a work area beyond what is free (both before anything is queued, the message names the sizes), an R that is not finite,
 * more than 40 squarings.  Waits for the row sums, then asynchronous on the context's stream. */
int sr_symm_expm_f64_dev(sr_ctx *, const double *R, int64_t P, const double *tau_host, int64_t n_tau, double *out);
/* the arithmetic of the scaling alone (a host function, no context): s = the least integer >= 0 with norm1 tau / 2^s <= 0.5,
 * products = 11 + s.  -3: norm1 or tau not finite or negative, s > 40. */
int sr_symm_expm_plan(double norm1, double tau, int *s, int *products);
/* What sr_symm_expm_f64_dev refuses for its sizes, with the results counted against the FREE memory as well: for a caller that has
 * yet to allocate out.  Allocates and queues nothing. */
int sr_symm_expm_check(sr_ctx *, int64_t P, int64_t n_tau);

/* ---- time-lagged P2 cross-correlation between pairs of vectors (sr_ct_cross.hip; beyond the reference) ---------------------------
 * For pair p = (i, j) = (pair_i[p], pair_j[p]) on the Palmer chunk table of kernel 1 (R chunks of F frames, chunk_start_host as there):
 *     S_ij[k] = sum_{t = 0}^{F - 1 - k} (u_i(t) . u_j(t + k))^2,      k = 0 .. L = F / 2,   per chunk
 *     C_ij(k) = mean over the chunks of 1.5 S_ij[k] / (F - k) - 0.5   (k = 1 .. L),   dC = std over the chunks / (sqrt(R) - 1)
 * -- what every cross-correlated relaxation rate computed from a trajectory starts from (the two C-H dipoles of a methylene group,
 * N-H against CA-HA, a dipole against a CSA axis).  sym = 1: S is (S_ij + S_ji) / 2, the symmetric function relaxation theory uses
 * (for i = j: the autocorrelation, to rounding); sym = 0: S_ij alone -- the later frame belongs to j; C_ji is the pair (j, i).
 * Arithmetic and modes as the direct form of kernel 1 (mode 0: float32 dot products, short float32 partial sums folded into float64;
 * mode 1: float64 throughout); no atomics, equal input gives bit-equal output.  Mean and dC come from kernel 1's own reduction over
 * the chunks (the raw sums have its layout, pairs in the place of vectors), so R = 1 gives the dC it gives.
 *   P0  (nP)     equal-time <P2(u_i . u_j)>: mean over the chunks of 1.5 S[0] / F - 0.5, the rigid-limit P2(cos theta_ij)
 *   dP0 (nP)     its error over the chunks by the same formula as dC (optional, may be NULL)
 *   Ct, dCt      (L, nP) float64, lags 1 .. L like kernel 1
 * One workgroup stages both series of a (pair, chunk) in LDS, 24 bytes per frame: F up to sr_ct_cross_max_frames() (6624 with the
 * 160 KiB of gfx950); a longer chunk is refused with -4 (the sr_*ct_cross_long_* functions below take it).  The pair tables are HOST arrays, consumed on
 * return; an index outside [0, nV) is refused with -3.  Every refusal comes before anything is launched.
 * _dev: packed planes in, P0 / dP0 / Ct / dCt DEVICE arrays, asynchronous behind the upload of the tables; psum_ws (optional, may be NULL):
 * (nP, R, sr_ct_psum_stride(F)) float64 raw sums, S[0] in slot 0.  sr_vectors_: kernel 0 once per object, results on the HOST, blocking; _err_ is the same call
 * with dP0 as well. */
int64_t sr_ct_cross_max_frames(sr_ctx *);
int sr_ct_cross_f32_dev(sr_ctx *, const float *soa, int64_t Npad, int64_t nV, int64_t R, int64_t F, const int64_t *chunk_start_host,
                        const int32_t *pair_i_host, const int32_t *pair_j_host, int64_t nP, int sym, int mode, double *psum_ws,
                        double *P0, double *dP0, double *Ct, double *dCt);
int sr_vectors_ct_cross_f32(sr_ctx *, sr_vectors *, int64_t R, int64_t F, const int64_t *chunk_start_host,
                            const int32_t *pair_i, const int32_t *pair_j, int64_t nP, int sym, int mode,
                            double *P0, double *Ct, double *dCt);
int sr_vectors_ct_cross_err_f32(sr_ctx *, sr_vectors *, int64_t R, int64_t F, const int64_t *chunk_start_host,
                                const int32_t *pair_i, const int32_t *pair_j, int64_t nP, int sym, int mode,
                                double *P0, double *dP0, double *Ct, double *dCt);

/* The same functions for longer chunks (sr_ct_cross_long.hip): the blocked transforms of kernel 1's long form on the two series of a
 * pair, 5462 <= F <= sr_ct_cross_long_max_frames() = 262144 frames per chunk; a longer chunk is refused with -4, a shorter one with -3,
 * a pair index outside the vectors with -3, all before anything is launched.  Arguments and results as the functions above.  Mode 0:
 * float32 block transforms (once per (vector, chunk) that the pairs name), float64 from the cross-spectra on, lag 0 a float64 sum;
 * mode 1: the definition in float64, lag by lag.  No atomics: equal input gives bit-equal output, whatever "ct_long_ws_mb" tiles.
 * Each entry point runs its own kernel at every length it takes; choosing between the two is the caller's (spinrelax_amd/ct.py goes by
 * sr_set_option("ct_cross_long_min_frames", F0): 5462 .. 262144, default 6625, the first length the functions above refuse). */
int64_t sr_ct_cross_long_max_frames(sr_ctx *);
int sr_ct_cross_long_f32_dev(sr_ctx *, const float *soa, int64_t Npad, int64_t nV, int64_t R, int64_t F, const int64_t *chunk_start_host,
                             const int32_t *pair_i_host, const int32_t *pair_j_host, int64_t nP, int sym, int mode, double *psum_ws,
                             double *P0, double *dP0, double *Ct, double *dCt);
int sr_vectors_ct_cross_long_f32(sr_ctx *, sr_vectors *, int64_t R, int64_t F, const int64_t *chunk_start_host,
                                 const int32_t *pair_i, const int32_t *pair_j, int64_t nP, int sym, int mode,
                                 double *P0, double *Ct, double *dCt);
int sr_vectors_ct_cross_long_err_f32(sr_ctx *, sr_vectors *, int64_t R, int64_t F, const int64_t *chunk_start_host,
                                     const int32_t *pair_i, const int32_t *pair_j, int64_t nP, int sym, int mode,
                                     double *P0, double *dP0, double *Ct, double *dCt);

/* ---- distance-weighted dipolar correlation function of a flexible spin pair (sr_ct_dipolar.hip; beyond the reference) -----------------
 * Every function above takes the inter-spin vector as a unit vector: right for a bonded N-H or C-H pair.  Between two spins whose
 * distance fluctuates with the orientation (an inter-proton NOE, a methyl proton against a backbone proton, a ligand-protein contact)
 * the relaxation-active function is
 *     C_dd(k) = < P2(u(t) . u(t+k)) r(t)^-3 r(t+k)^-3 > / < r^-6 >
 * (Brueschweiler et al., J. Am. Chem. Soc. 114, 2289 (1992); Peter, Daura & van Gunsteren, J. Biomol. NMR 20, 297 (2001)), on the Palmer
 * chunk table of kernel 1 (R chunks of F frames, chunk_start_host as there).  Per vector, r_ref = min over the frames held of r(t),
 * w(t) = (r_ref / r(t))^3 in (0, 1], a(t) = u(t) sqrt(w(t)); P2(u . u') w w' = 1.5 (a . a')^2 - 0.5 w w'.  Per chunk r
 *     c_r(k) = [1.5 sum_t (a(t) . a(t+k))^2 - 0.5 sum_t w(t) w(t+k)] / (F - k),     n_r = sum_t w(t)^2 / F
 *     C_dd(k) = mean_r c_r(k) / mean_r n_r   (a ratio of chunk means; C_dd(0) = 1),   k = 1 .. L = F / 2
 *     dC_dd(k) = [std_r c_r(k) / (sqrt(R) - 1)] / mean_r n_r   -- the scatter of the normaliser itself is ignored
 * Mean and std of c_r come from kernel 1's own reduction over the chunks, so R = 1 gives the dC it gives.  Arithmetic and modes as the
 * direct form of kernel 1 (mode 0: float32 products, float32 partial sums of at most 16 terms folded into float64; mode 1: float64
 * throughout); no atomics, equal input gives bit-equal output.
 *   sr_pack_dipolar_f32_dev  frame-major vectors (N, Vtot, 3) float32 of ANY length, columns [v0, v0 + nV) -> four planes per vector
 *                            a_x, a_y, a_z, w in kernel 0's layout, planes[(v * 4 + c) * Npad + n], zero for n in [N, Npad), and
 *                            r_ref (nV) float64.  dist_dev (N, Vtot) float32, optional: when given it holds the distances and the
 *                            vectors only give the direction; when NULL the length of a vector is the distance.  float64 arithmetic,
 *                            rounded once to float32.  A vector with a frame that is not finite, or whose direction is (0, 0, 0),
 *                            gets r_ref = NaN; a zero-length vector without dist_dev gives r_ref = 0.  Asynchronous.
 *   sr_ct_dipolar_f32_dev    those planes -> Ct, dCt (L, nV) float64 and wmean (nV, 2) = <w>, <w^2> over the frames of all chunks, DEVICE
 *                            arrays; psum_ws (optional, may be NULL): (nV, R, sr_ct_psum_stride(F)) float64.  Asynchronous (behind the
 *                            upload of a chunk table); every argument check comes before the first launch.
 *   sr_vectors_ct_dipolar_f32  the same of resident vectors, results on the HOST, blocking: Ct, dCt (L, nV) and per vector
 *                            reff6 = r_ref <w^2>^(-1/6) = <r^-6>^(-1/6),  reff3 = r_ref <w>^(-1/3) = <r^-3>^(-1/3) and the radial order
 *                            parameter S2rad = <w>^2 / <w^2>, in the units of the input.  dist_host (frames held, nV) float32, optional,
 *                            as dist_dev above; an entry <= 0 or not finite is refused (-3), and so is, after the r_ref pass and by
 *                            name, a vector whose r_ref is <= 0 or not finite.  The four-plane pack is the object's own: it is kept
 *                            like the three planes of the other analyses, dropped by the same events (append, truncate) and does not
 *                            disturb them; a pack made with dist_host is never reused (the array is the caller's).
 * One workgroup stages the four series of a (vector, chunk) in LDS, 16 bytes per frame: F up to sr_ct_dipolar_max_frames() (10016 with the
 * 160 KiB of gfx950); a longer chunk is refused with -4 before anything is launched and belongs to the blocked form below. */
int64_t sr_ct_dipolar_max_frames(sr_ctx *);
int sr_pack_dipolar_f32_dev(sr_ctx *, const float *vecs_dev, const float *dist_dev, int64_t N, int64_t Vtot, int64_t v0, int64_t nV,
                            float *planes_dev, int64_t Npad, double *rref_dev);
int sr_ct_dipolar_f32_dev(sr_ctx *, const float *planes_dev, int64_t Npad, int64_t nV, int64_t R, int64_t F, const int64_t *chunk_start_host,
                          int mode, double *psum_ws, double *Ct, double *dCt, double *wmean);
int sr_vectors_ct_dipolar_f32(sr_ctx *, sr_vectors *, const float *dist_host, int64_t R, int64_t F, const int64_t *chunk_start_host, int mode,
                              double *Ct, double *dCt, double *reff6, double *reff3, double *S2rad);

/* ---- distance-weighted cross-correlation between pairs of flexible spin pairs (sr_ct_dipolar_cross.hip; beyond the reference) --------
 * The two functions above at once, what dipole-dipole cross-correlated relaxation between two spin pairs of fluctuating distance needs:
 *     C_ij(k) = < P2(u_i(t) . u_j(t+k)) r_i(t)^-3 r_j(t+k)^-3 > / sqrt(< r_i^-6 > < r_j^-6 >),   k = 1 .. L = F / 2
 * and P0 = C_ij(0), from the four planes of sr_pack_dipolar_f32_dev and a pair table as sr_ct_cross_f32_dev takes it (HOST arrays, consumed
 * on return; the later frame from vector j; sym = 1: the mean of C_ij and C_ji, sym = 0: C_ij alone; mode as there).  Per chunk r
 *     c_r(k) = [1.5 sum_t (a_i(t) . a_j(t+k))^2 - 0.5 sum_t w_i(t) w_j(t+k)] / (F - k),     n_v = mean_r sum_t w_v(t)^2 / F
 *     C_ij(k) = mean_r c_r(k) / sqrt(n_i n_j),   dC_ij(k) = [std_r c_r(k) / (sqrt(R) - 1)] / sqrt(n_i n_j);   P0 and dP0 alike from c_r(0)
 * (ratios of chunk means: the scatter of the normaliser is ignored, the r_ref factors cancel).  For i = j: C_dd of sr_ct_dipolar_f32_dev
 * and P0 = 1, to rounding.  No atomics: equal input gives bit-equal output, a repeated pair the same bits.
 *   sr_ct_dipolar_cross_f32_dev       planes (nV, 4, Npad) -> P0, dP0 (nP; dP0 may be NULL), Ct, dCt (L, nP) and wsum2 (nP, R, 2) = the sums
 *                                     of w_i^2 and w_j^2 over every chunk, float64 DEVICE arrays; psum_ws (optional, may be NULL):
 *                                     (nP, R, sr_ct_psum_stride(F)) float64.  Asynchronous behind the upload of the small tables; every
 *                                     argument check comes before the first launch.
 *   sr_vectors_ct_dipolar_cross_f32   the same of resident vectors, results on the HOST, blocking, and reff6 (nP, 2) = <r^-6>^(-1/6) of the
 *                                     two vectors of each pair over the frames of the chunks, in the units of the input.  dist_host, its
 *                                     refusals and the reuse of the object's four-plane pack exactly as sr_vectors_ct_dipolar_f32.
 * One workgroup stages the eight series of a (pair, chunk) in LDS, 32 bytes per frame: F up to sr_ct_dipolar_cross_max_frames() (4896 with
 * the 160 KiB of gfx950); a longer chunk is refused with -4 before anything is launched and belongs to the blocked form below.  A pair
 * index or a chunk start outside what is held, a bad mode or sym: -3. */
int64_t sr_ct_dipolar_cross_max_frames(sr_ctx *);
int sr_ct_dipolar_cross_f32_dev(sr_ctx *, const float *planes_dev, int64_t Npad, int64_t nV, int64_t R, int64_t F, const int64_t *chunk_start_host,
                                const int32_t *pair_i_host, const int32_t *pair_j_host, int64_t nP, int sym, int mode, double *psum_ws,
                                double *P0, double *dP0, double *Ct, double *dCt, double *wsum2);
int sr_vectors_ct_dipolar_cross_f32(sr_ctx *, sr_vectors *, const float *dist_host, int64_t R, int64_t F, const int64_t *chunk_start_host,
                                    const int32_t *pair_i, const int32_t *pair_j, int64_t nP, int sym, int mode, double *P0, double *dP0,
                                    double *Ct, double *dCt, double *reff6);

/* ---- the two distance-weighted functions for long chunks: blocked transforms (sr_ct_dipolar_long.hip) -----------------------------------
 * The same functions, arguments and results as the four entry points above for chunks of up to sr_ct_dipolar_long_max_frames() =
 * sr_ct_dipolar_cross_long_max_frames() = 262144 frames, by the blocked float32 transforms of kernel 1's long-chunk form on the five
 * traceless signals of a: with |a|^2 = w, 1.5 (a . a')^2 - 0.5 w w' = 1.5 Q : Q', Q = a (x) a - (|a|^2 / 3) I.  |a|^2 = w holds to the
 * float32 rounding of the pack, so the planes MUST come from sr_pack_dipolar_f32_dev (the difference to the definition on such planes:
 * 1.5e-9 of C); on other four-plane input the result is Q : Q', not the definition.  The normalisers and the distance outputs come
 * from the w plane in float64, and so does lag 0 of a pair.  mode 1: the definition from the planes in float64, one thread per lag
 * (the on-device check, slow).  No atomics: equal input gives bit-equal output whatever the tiling of the work area (option
 * "ct_long_ws_mb"), a repeated pair the same bits.
 * Every argument check comes before the first launch: -4 beyond 262144 frames per chunk, -3 below 5462 (pair form: 4097) frames, where
 * the block structure would leave what the shared kernels are tested at, and -3 / -2 for what the direct forms refuse so.  The entry
 * points do not dispatch: each runs its own kernels.  spinrelax_amd/ct.py gives a chunk to the blocked form when the direct one
 * cannot stage it or when it has at least "ct_dipolar_long_min_frames" (default 10017, 5462 .. 262144) / "ct_dipolar_cross_long_min_frames"
 * (default 4897, 4097 .. 262144) frames (sr_set_option). */
int64_t sr_ct_dipolar_long_max_frames(sr_ctx *);
int64_t sr_ct_dipolar_cross_long_max_frames(sr_ctx *);
int sr_ct_dipolar_long_f32_dev(sr_ctx *, const float *planes_dev, int64_t Npad, int64_t nV, int64_t R, int64_t F, const int64_t *chunk_start_host,
                               int mode, double *psum_ws, double *Ct, double *dCt, double *wmean);
int sr_vectors_ct_dipolar_long_f32(sr_ctx *, sr_vectors *, const float *dist_host, int64_t R, int64_t F, const int64_t *chunk_start_host, int mode,
                                   double *Ct, double *dCt, double *reff6, double *reff3, double *S2rad);
int sr_ct_dipolar_cross_long_f32_dev(sr_ctx *, const float *planes_dev, int64_t Npad, int64_t nV, int64_t R, int64_t F,
                                     const int64_t *chunk_start_host, const int32_t *pair_i_host, const int32_t *pair_j_host, int64_t nP, int sym,
                                     int mode, double *psum_ws, double *P0, double *dP0, double *Ct, double *dCt, double *wsum2);
int sr_vectors_ct_dipolar_cross_long_f32(sr_ctx *, sr_vectors *, const float *dist_host, int64_t R, int64_t F, const int64_t *chunk_start_host,
                                         const int32_t *pair_i, const int32_t *pair_j, int64_t nP, int sym, int mode, double *P0, double *dP0,
                                         double *Ct, double *dCt, double *reff6);

/* ---- bond-vector correlation function split into the five tumbling modes of an anisotropic diffusion tensor (sr_ct_modes.hip; beyond
 * the reference) ----
 * The reference's anisotropic J(w) multiplies a static histogram of the vector's orientation in the principal-axis frame by one internal
 * C(t) shared by the five modes: exact only if the internal motion decays every mode alike.  This is sr_noe_modes' definition with
 * w = 1, on the Palmer chunk table of kernel 1 (R chunks of F frames, chunk_start_host as there) and at every lag of a chunk.  With
 * F = R(frame_quat), the constant rotation into the principal-axis frame of the tensor (--vecRot's convention), u(t) = F v(t) / |v(t)|:
 *     s0 = u_z^2 - 1/3,  s1 = u_x^2 - u_y^2,  s2 = u_y u_z,  s3 = u_x u_z,  s4 = u_x u_y
 * and per chunk r and lag k = 0 .. L = F / 2, <.> = sum_t / (F - k) over the origins t with t + k inside the chunk, s' taken at t + k:
 *     H0 = <s0 s0'>,  H1 = <s1 s1'>,  H2 = <s0 s1' + s1 s0'> / 2,  H3 = <s2 s2'>,  H4 = <s3 s3'>,  H5 = <s4 s4'>
 * the order of sr_noe_modes.  They do not depend on the tensor: one H serves any D (spinrelax_amd/noe.py: mode_amplitudes;
 * spinrelax_amd/modes.py: amplitudes, J, relaxation).  2.25 H0 + 0.75 H1 + 3 (H3 + H4 + H5) is kernel 1's C(k) whatever the frame.
 * H (L + 1, nV, 6) is the mean over the chunks, lag 0 included (a_m(0) is the mode amplitude); dH its std / (sqrt(R) - 1), kernel 1's
 * convention, so R = 1 gives what it gives; smean (nV, 5) the means of the five signals over the frames of all chunks used, whose
 * products (m0^2, m1^2, m0 m1, m2^2, m3^2, m4^2) are the six sums of the plateaus.
 * Arithmetic as the direct form of kernel 1.  mode 0: float32 FMAs, float32 partial sums of at most 16 signed terms started at zero,
 * folded into float64; mode 1: the same definition in float64 from the planes (the on-device check, not built for speed).  No atomics:
 * equal input gives bit-equal output, and a vector's bits do not depend on the other vectors of the call.
 *   sr_pack_modes_f32_dev    frame-major vectors (N, Vtot, 3) float32 of ANY positive length, columns [v0, v0 + nV) -> five planes per
 *                            vector s0 .. s4 in kernel 0's layout, planes[(v * 5 + c) * Npad + n], zero for n in [N, Npad).  F is formed
 *                            on the host in float64; F and the normalisation are applied in float64, each value rounded once to float32.
 *                            frame_quat_host: HOST (4) float64 (w, x, y, z), a unit quaternion (normalised again before use), or NULL
 *                            (F = 1).  bad_dev (nV) int32: 1 for a vector with a frame that is not finite or of zero length (its planes
 *                            hold zeros there), else 0.  Asynchronous.  Refused with -3 before anything is queued: a bad shape; a frame
 *                            quaternion that is not finite or whose squared norm is farther than 1e-6 from 1 (sr_noe_modes' rule).
 *   sr_ct_modes_f32_dev      those planes -> H, dH (L + 1, nV, 6) and smean (nV, 5), float64 DEVICE arrays; psum_ws (optional, may be
 *                            NULL): (6 nV, R, sr_ct_psum_stride(F)) float64.  Asynchronous (behind the upload of a chunk table); every
 *                            argument check comes before the first launch.
 *   sr_vectors_ct_modes_f32  the same of resident vectors, results on the HOST, blocking.  The pack depends on the frame: it is a work
 *                            area of the call, not kept on the object.  A vector that the pack marks bad is refused (-3) by name.
 * One workgroup stages the five series of a (vector, chunk) in LDS, 20 bytes per frame: F up to sr_ct_modes_max_frames() (7968 with the
 * 160 KiB of gfx950); a longer chunk is refused with -4 before anything is queued (this function has only the staged form); a chunk start outside
 * what is held, a bad shape or mode: -3.  The context stays usable after every refusal. */
int64_t sr_ct_modes_max_frames(sr_ctx *);
int sr_pack_modes_f32_dev(sr_ctx *, const float *vecs_dev, int64_t N, int64_t Vtot, int64_t v0, int64_t nV, const double *frame_quat_host,
                          float *planes_dev, int64_t Npad, int32_t *bad_dev);
int sr_ct_modes_f32_dev(sr_ctx *, const float *planes_dev, int64_t Npad, int64_t nV, int64_t R, int64_t F, const int64_t *chunk_start_host,
                        int mode, double *psum_ws, double *H, double *dH, double *smean);
int sr_vectors_ct_modes_f32(sr_ctx *, sr_vectors *, const double *frame_quat_host, int64_t R, int64_t F, const int64_t *chunk_start_host,
                            int mode, double *H, double *dH, double *smean);

/* ---- kernel 3b: multi-exponential C(t) model --------------------------------------------
 * Model of curvefit_exponential (fitting_Ct_functions.py:419-427): params = [C_1..C_K, tau_1..tau_K
 * (, S2)], P = 2K or 2K+1; even P: S2 = 1 - sum C.  resid = (model - C)/sigma (sigma may be NULL),
 * jac[i,l,p] = d resid[i,l] / d param[i,p] (analytic).  All arrays row-major float64. */
int sr_expfit_resjac_f64(sr_ctx *, const double *t /*[nRes,L]*/, const double *C, const double *sigma,
                         const double *params /*[nRes,P]*/, int nRes, int L, int P,
                         double *resid /*[nRes,L]*/, double *jac /*[nRes,L,P] or NULL*/);
/* Test-facing probe of the fit kernels' evaluations: for each residue, ONE evaluation at params x (nRes,P) of what the solver
 * evaluates at an iterate, by the same device code (Residue::stage, eval_f with its point cache, eval_jac; sr_fit.hip) at the bounds
 * the solver builds from tau_max, under the context's fit_waves / fit_lds / fit_geo.  Outputs (host pointers): geo (nRes) whether
 * the uniform-grid products were taken; cost (nRes) 0.5 f.f, NaN when a residual is not finite; f (nRes,L) the residuals
 * (model - C)/sigma; JtJ (nRes,P,P) and Jtf (nRes,P) of the Jacobian (jac_mode 0: scipy's 2-point forward differences, 1: analytic);
 * dx (nRes,P) the forward-difference steps (x + h) - x. */
int sr_expfit_probe_f64(sr_ctx *, const double *t, const double *C, const double *sigma, const double *x, int nRes, int L, int P,
                        double tau_max, int jac_mode, int *geo, double *cost, double *f, double *JtJ, double *Jtf, double *dx);
/* Test-facing probe of ONE trust-region step of the fit kernels: for each of nRes cases, what one pass of the solver's outer loop
 * computes between the Jacobian and the trial evaluation, by the solver's own device code (Coleman-Li scaling, B = D A D + diag(g dv),
 * solve_tr, select_step, strictly_feasible; sr_fit.hip), from x (nRes,P), JtJ (nRes,P,P; the lower triangle is read), Jtf (nRes,P),
 * the radius Delta (nRes), the Levenberg parameter alpha carried over (nRes), m (nRes; the number of data points of the rank test) and
 * the bounds the solver builds from tau_max.  No residue data.  mode 0 "step", outputs (host pointers): vec (nRes,8,P) = v, dv, d,
 * g_h, p_h of solve_tr, step, step_h, xn after strictly_feasible(., 0); B (nRes,P,P); sca (nRes,8) = g_norm, theta, alpha after
 * solve_tr, predicted, |step_h|, |step|, Delta, 0; flags (nRes,4) = solve_tr took the full-rank path, the branch of select_step
 * (0 in bounds, 1 theta * step to the bound, 2 reflected, 3 Cauchy), factorisations of B + alpha I that met a non-positive pivot,
 * passes of the alpha iteration.  mode 1 "init": vec rows 0, 1, 7 = v, dv and x after strictly_feasible(., 1e-10), sca[6] = the
 * initial radius; everything else 0. */
int sr_expfit_step_probe_f64(sr_ctx *, const double *x, const double *JtJ, const double *Jtf, const double *Delta,
                             const double *alpha, const int *m, int nRes, int P, double tau_max, int mode, double *vec, double *B,
                             double *sca, int *flags);
/* Batched bounded least-squares fit, one workgroup per residue, whole solve on the device
 * (replaces the scipy curve_fit call of conduct_curve_fitting, fitting_Ct_functions.py:322-324:
 * bounds 0 <= C,S2 <= 1, 0 <= tau <= tau_max).  p0 in / popt out (nRes,P); pcov (nRes,P,P) is the
 * curve_fit covariance (J^T J)^-1 * 2 cost/(L-P); chisq = mean(resid_unweighted^2 / sigma)
 * (calc_chiSq, :272-276); status per residue: >0 converged (1 gtol, 2 ftol, 3 xtol), 0 max iterations,
 * <0 failure.  Host pointers. */
int sr_expfit_lm_f64(sr_ctx *, const double *t, const double *C, const double *sigma, int nRes, int L, int P,
                     const double *p0, double tau_max, int max_iter,
                     double *popt, double *pcov, double *chisq, int *status, int *n_iter);
/* device-pointer form; skip (nRes bytes, device, may be NULL): residues with skip[i] != 0 are left
 * untouched (used by the host-side model-order search, which stops residues individually);
 * max_iter < 0 selects the analytic Jacobian instead of scipy's 2-point differences;
 * work (device, nRes*2*L doubles, may be NULL = context-owned): residual scratch; pass one buffer per
 * concurrently running launch when fits are enqueued on several streams. */
int sr_expfit_lm_f64_dev(sr_ctx *, const double *t, const double *C, const double *sigma, int nRes, int L, int P,
                         const double *p0, double tau_max, int max_iter, const unsigned char *skip, double *work,
                         double *popt, double *pcov, double *chisq, int *status, int *n_iter);

/* The whole model-order search of optimised_curve_fitting (fitting_Ct_functions.py:278-304) in ONE launch, one
 * workgroup per residue: for every order in `orders` (numbers of parameters, e.g. 2,3,5,7,9; host array, at most 8)
 * the initial guess of initialise_for_fit_advanced (:359-374), the bounded fit of conduct_curve_fitting (:306-345),
 * its three quality flags and the accept / reject rule (chi_threshold = chiSqThreshold, 0.5 in the reference).
 * All other pointers are DEVICE pointers.
 *   tau_guess   (tau_guess_rows, sum orders[j]/2): the log-spaced tau guesses of :361-362 for every order, one after
 *               the other; tau_guess_rows = 1 (every residue has the same time axis) or nRes
 *   work        (nRes*L doubles) or NULL: only used when a residue (3*L doubles) does not fit into LDS
 *   popt, dP    (nOrders, nRes, Pmax) with Pmax = max(orders): optimum and sqrt(diag(pcov)) of every attempted order
 *   chisq       (nOrders, nRes) calc_chiSq of the fit, +inf when the solver failed
 *   status,nfev (nOrders, nRes); status = -100: order not attempted (the search had already stopped)
 *   best        (nRes) index into orders of the accepted model, -1 = no satisfactory fit
 *   sel_*       the accepted model with its components sorted by tau (sort_components :203-209): S2 (nRes),
 *               C and tau (nRes, Pmax/2; unused entries 0 and 1), chi (nRes, NaN if none), K (nRes) = components
 * The launch is asynchronous on the context's stream. */
int sr_expfit_order_search_f64_dev(sr_ctx *, const double *t, const double *C, const double *sigma, int nRes, int L,
                                   const int *orders, int nOrders, const double *tau_guess, int tau_guess_rows,
                                   double tau_max, double chi_threshold, double *work, double *popt, double *dP,
                                   double *chisq, int *status, int *nfev, int *best, double *sel_S2, double *sel_C,
                                   double *sel_tau, double *sel_chi, int *sel_K);
/* The same for SEVERAL batches of residues in one launch (the pipeline merges the searches of a group of trajectory shards:
 * the per-residue loop of calculate-fitted-Ct.py:161-178 over all of them).  A launch lasts as long as its slowest residue and a
 * residue's cost is not known beforehand (2 to 9 parameters, 20 to 900 function evaluations): merged launches keep the chip
 * full while the stragglers of every batch run.
 *   t_rows          1: one time axis (L values) shared by every residue; nRes: a row per residue as above
 *   dispatch_order  DEVICE, nRes residue indices, or NULL: workgroup b solves residue dispatch_order[b].  Results are stored
 *                   at the residue's own index whatever the order; a permutation spreads residues that are expensive for the
 *                   same reason (the same position in every batch) over the chip instead of over one part of it.
 *   tail_signal     NULL, or a signal (sr_signal_alloc): the launch's last workgroup stores tail_value there when it STARTS.
 *                   Workgroups start in index order, so from that moment every residue has been handed to a CU and the launch
 *                   only drains -- slots free up while the longest fits finish.  A stream that waits for the value
 *                   (sr_stream_wait_signal) starts its bandwidth-bound kernels exactly then. */
int sr_expfit_order_search_batched_f64_dev(sr_ctx *, const double *t, int t_rows, const double *C, const double *sigma, int nRes,
                                           int L, const int *orders, int nOrders, const double *tau_guess, int tau_guess_rows,
                                           double tau_max, double chi_threshold, const int *dispatch_order,
                                           uint32_t *tail_signal, uint32_t tail_value, double *work,
                                           double *popt, double *dP, double *chisq, int *status, int *nfev, int *best,
                                           double *sel_S2, double *sel_C, double *sel_tau, double *sel_chi, int *sel_K);
/* The batched search fed with kernel 1's RAW SUMS instead of finished C(t) / dC(t): every workgroup computes the chunk statistics of
 * its residue (the arithmetic of sr_ct_finalize_f64_dev, bit for bit) while it stages it, so no sr_ct_finalize launch -- a pure
 * bandwidth pass -- runs in front of a kernel that leaves the memory system idle.
 *   sums        DEVICE (nRes, R, sr_ct_psum_stride(F)) as sr_ct_palmer_sums_f32_dev writes them, series in the place of residues
 *   R, F        chunks and frames per chunk; L must be F / 2
 *   CtT, dCtT   DEVICE (nRes, L), OUTPUT: C(t) and dC(t), residue-major (what sr_ct_finalize_t_f64_dev writes there); final when
 *               the launch has ended.  The (lags, vectors) arrays follow by sr_transpose_batched_f64_dev.
 * Every other argument as above; with dispatch_order the sums row, the output rows and the tau guesses all follow the residue.
 * Refused before anything is queued: a null sums / CtT / dCtT -2; R < 1, F < 2 or L != F / 2 -3; then the checks above. */
int sr_expfit_order_search_sums_f64_dev(sr_ctx *, const double *t, int t_rows, const double *sums, int64_t R, int64_t F,
                                        double *CtT, double *dCtT, int nRes, int L, const int *orders, int nOrders,
                                        const double *tau_guess, int tau_guess_rows, double tau_max, double chi_threshold,
                                        const int *dispatch_order, uint32_t *tail_signal, uint32_t tail_value, double *work,
                                        double *popt, double *dP, double *chisq, int *status, int *nfev, int *best, double *sel_S2,
                                        double *sel_C, double *sel_tau, double *sel_chi, int *sel_K);
/* sr_expfit_order_search_f64_dev with HOST pointers throughout (staged through the context's work space, synchronous) */
int sr_expfit_order_search_f64(sr_ctx *, const double *t, const double *C, const double *sigma, int nRes, int L,
                               const int *orders, int nOrders, const double *tau_guess, int tau_guess_rows,
                               double tau_max, double chi_threshold, double *popt, double *dP, double *chisq,
                               int *status, int *nfev, int *best, double *sel_S2, double *sel_C, double *sel_tau,
                               double *sel_chi, int *sel_K);

/* ---- kernel 3a: J(omega) and R1/R2/NOE/rho ----------------------------------------------
 * sr_jomega_f64: elementwise x/(x*x+y*y), the double loop of Jomega/Jomega.c:49-66, evaluated on the
 * GPU (host pointers; n elements, both inputs already broadcast by the caller). */
int sr_jomega_f64(sr_ctx *, const double *x, const double *y, double *out, int64_t n);

/* Batched relaxation.  Replaces _obtain_R1R2NOErho / _obtain_Jomega
 * (calculate-relaxations-from-Ct.py:82-191) and the class API spinRelaxationR1/R2/NOE.eval
 * (spectral_densities.py:820-907) for E "experiments" (field settings) at once.
 *   model        0 direct transform (J_direct_transform, spectral_densities.py:2024-2033)
 *                1 rigid sphere, D[0] = Diso (J_combine_isotropic_exp_decayN, :2038-2050)
 *                2 symmetric top, D[0] = Dpar, D[1] = Dperp (J_combine_symmtop_exp_decayN, :2057-2077)
 *                3 fully anisotropic (rhombic) ellipsoid, D = {Dx, Dy, Dz}: the principal values in any order, along the x, y, z
 *                  axes of the frame the vectors are given in (Woessner 1962; Ghose, Fushman & Cowburn 2001).  Five rates
 *                  4Dx+Dy+Dz, Dx+4Dy+Dz, Dx+Dy+4Dz, 6Diso +- 6R and five amplitudes per vector; no counterpart in the
 *                  reference, whose helpers for this model (:1908-1932) do not work.  Needs vectors like model 2.
 *   omega        (E,5): [0, wX, wH-wX, wH, wH+wX] in 1/time-unit
 *   f_DD (E), f_CSA (E,nRes), time_fact (E), gamma_ratio (E) = gamma_H/gamma_X
 *   S2 (nRes), C/tau (nRes,Kmax) with nComps (nRes) valid entries -- already zeta-scaled
 *   binvecs (B,3) unit vectors shared by every residue (bin centres) or (nRes,3) when B == 0 (models 2 and 3)
 *   weights (nRes,B) or NULL (uniform); a DEVICE pointer when weights_on_device != 0 (the histogram
 *                kernel 2 left in HBM), otherwise a host pointer
 *   noe_mode     0: NOE from the per-vector R1 (old API, :1706/:1722)
 *                1: NOE from the vector-averaged R1 (new API, :881-892)
 *   out          (E, nRes, 4, 2): {R1,R2,NOE,rho} x {weighted mean, weighted sigma}; sigma = 0 when B == 0
 *   Jout         (E, nRes, 5, 2) weighted mean/sigma of J(omega) or NULL (the --Jomega output)
 *   stats        (E, nRes, 12) or NULL: sufficient statistics for CSA fitting.  The CSA enters the rates only
 *                through f_CSA (proportional to csa^2): R1 = a1 + f_CSA*b1, R2 = a2 + f_CSA*b2 per vector, so
 *                [a1, b1, Var a1, Cov(a1,b1), Var b1, a2, b2, Var a2, Cov(a2,b2), Var b2, N, Var N]
 *                (weighted means / (co)variances over the vectors, N = 6 J(wH+wX) - J(wH-wX)) give the
 *                weighted mean AND sigma of R1, R2 and the new-API NOE for ANY csa without touching the
 *                2 592 bins again (rsCSA optimiser, spectral_densities.py:1371-1382, 1430-1447).
 * Host pointers. */
int sr_jomega_relax_f64(sr_ctx *, int model, const double *D, int E, const double *omega, const double *f_DD,
                        const double *f_CSA, const double *time_fact, const double *gamma_ratio,
                        int nRes, int Kmax, const double *S2, const double *C, const double *tau, const int *nComps,
                        int B, const double *binvecs, const double *weights, int weights_on_device, int noe_mode,
                        double *out, double *Jout, double *stats);
/* Device-pointer form for a pipeline that never leaves the GPU: every array argument is a DEVICE pointer (D stays a
 * host array of 1, 2 or 3 numbers), nComps[i] must be within 0..Kmax (not checked), S2 and C are multiplied by zeta on
 * load (the reference scales the fitted model by zeta first, calculate-relaxations-from-Ct.py:747-750; pass 1.0 for
 * already-scaled input); asynchronous on the context's stream. */
int sr_jomega_relax_f64_dev(sr_ctx *, int model, const double *D, int E, const double *omega, const double *f_DD,
                            const double *f_CSA, const double *time_fact, const double *gamma_ratio,
                            int nRes, int Kmax, double zeta, const double *S2, const double *C, const double *tau,
                            const int *nComps, int B, const double *binvecs, const double *weights, int noe_mode,
                            double *out, double *Jout, double *stats);

/* Residue-specific CSA search of the new class API: replaces the per-residue fmin_powell loop of
 * spinRelaxationExperiments.optimisation_loop_do_local_step / optimisation_loop_do_local_step's objective
 * (spectral_densities.py:1371-1382, 1430-1447).  One device thread per residue runs scipy's one-variable Powell / Brent
 * search (restated from scipy/optimize/_optimize.py, see sr_relax.hip) over the closed forms the 12 statistics of
 * sr_jomega_relax_f64 give:
 *   stats (E, nRes, 12); column[e] = 0 R1, 1 R2, 2 NOE; csa_prefactor[e]: f_CSA = csa^2 * csa_prefactor[e];
 *   noe_factor[e] = time_fact * gamma_B / gamma_A, f_DD[e]; target / dtarget (E, nRes): the measured value and its
 *   uncertainty (0 when the file has none) of residue i in experiment e, read only where cover[e, i] != 0;
 *   has_err: the model values carry a sigma (vector distribution given); csa0 (nRes) start values; step = the initial
 *   direction (dictStepSizes['rsCSA']); xtol, ftol as fmin_powell's (1e-4 both in the reference's call).
 * Outputs: csa (nRes) = the LAST evaluated CSA of each search (what the reference keeps), values / errors (E, nRes) at
 * that CSA for covered entries (0 elsewhere), fopt (nRes) Powell's final objective, nfev (nRes) objective calls.
 * Residues no experiment covers keep csa0 and nfev = 0.  Host pointers. */
int sr_rscsa_search_f64(sr_ctx *, int E, int nRes, const double *stats, const int *column, const double *csa_prefactor,
                        const double *noe_factor, const double *f_DD, const double *target, const double *dtarget,
                        const unsigned char *cover, int has_err, const double *csa0, double step, double xtol, double ftol,
                        double *csa, double *values, double *errors, double *fopt, int *nfev);

/* Per-residue CSA refinement of the legacy single-field mode `--opt new`: replaces the loop of fmin_powell calls over
 * optfunc_R1R2NOE_new (calculate-relaxations-from-Ct.py:210-258, 935-1000), axisymmetric diffusion + vector histogram only (no ellipsoid:
 * the legacy modes stay as the reference has them).
 * One workgroup per residue runs scipy's one-variable Powell search (as sr_rscsa_search_f64); every objective call evaluates
 * R1, R2 and the old-API NOE over the B histogram bins with the arithmetic of sr_jomega_relax_f64 (noe_mode 0), casts value and
 * sigma to float32 like the reference's datablock and returns mean_k (model_k - exp_k)^2 / (sigma_exp_k^2 + sigma_model_k^2).
 *   D = {Dpar, Dperp}; omega (5); f_DD; gammaB0_sq = (gamma_X B0)^2 (f_CSA = 2/15 csa^2 gammaB0_sq); time_fact; gamma_ratio;
 *   S2 (nRes), C / tau (nRes, Kmax), nComps (nRes): the fitted models, already scaled by zeta; binvecs (B, 3), weights (nRes, B);
 *   expt (nRes, 3, 2): measured R1, R2, NOE and their uncertainties; csa0 (nRes) start values; step = Powell's initial
 *   direction (1.0: scipy's identity default), xtol, ftol (1e-4), maxiter, maxfun (1000: scipy's N * 1000).
 * Outputs (nRes): csa = Powell's optimum, fopt = the objective there, nfev = objective calls.  Host pointers. */
int sr_legacy_csa_search_f64(sr_ctx *, const double *D, const double *omega, double f_DD, double gammaB0_sq, double time_fact,
                             double gamma_ratio, int nRes, int Kmax, const double *S2, const double *C, const double *tau,
                             const int *nComps, int B, const double *binvecs, const double *weights, const double *expt,
                             const double *csa0, double step, double xtol, double ftol, int maxiter, int maxfun, double *csa,
                             double *fopt, int *nfev);

/* ---- trajectory front end ----------------------------------------
 * Replaces obtain_XHvecs (calculate-Ct-from-traj.py:64-86) with vecnorm_NDarray (transforms3d_supplement.py:40-52) and the
 * MDTraj center_coordinates + superpose(ref, frame=0, atom_indices=fit_indices) step between its two calls (:466-467):
 *   xyz       (nFrames, nAtoms, 3) float32 coordinates as MDTraj holds them (traj.xyz);
 *   idxX/idxH nV atom indices each (the X and H selections, same order), HOST arrays in both forms;
 *   fit_idx   nFit atom indices to superpose on, ref_xyz (nAtoms, 3) float32 reference coordinates, HOST arrays
 *             (both may be NULL when neither vec_fit nor quat is requested);
 *   vec_lab   (nFrames, nV, 3) float32 unit vectors (x_H - x_X)/|.| in float32 arithmetic, 0/0 -> 0: bit-identical to
 *             the reference's numpy expression; may be NULL;
 *   vec_fit   (nFrames, nV, 3) float32: the same bond rotated by the frame's optimal (unweighted least-squares, proper)
 *             rotation onto the reference, float64 inside, normalised; may be NULL;
 *   quat      (nFrames, 4) float64 (w, x, y, z), w >= 0: that rotation; may be NULL.
 * Both outputs have the (frames, vectors, 3) layout sr_pack_soa_f32_dev / sr_ct_palmer_f32 consume. */
int sr_xh_vectors_f32_dev(sr_ctx *, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *idxX_host,
                          const int32_t *idxH_host, int nV, const int32_t *fit_idx_host, int nFit, const float *ref_xyz_host,
                          float *vec_lab, float *vec_fit, double *quat);
int sr_xh_vectors_f32(sr_ctx *, const float *xyz, int64_t nFrames, int64_t nAtoms, const int32_t *idxX, const int32_t *idxH,
                      int nV, const int32_t *fit_idx, int nFit, const float *ref_xyz, float *vec_lab, float *vec_fit,
                      double *quat);

/* ---- global rotational diffusion: difference-quaternion lag correlations ----------
 * Replaces the per-lag reductions of calculate-dq-distribution.py: obtain_self_dq (:102-109, dq_i = q_i^-1 * q_{i+d} with
 * quat_mult_simd / quat_invert / quat_reduce_simd of transforms3d_supplement.py:163-186, 219-227), average_LegendreP1quat
 * (:111-112), average_anisotropic_tensor (:118-126) and their *_chunk variants (:128-144) inside the main loop :554-609.
 *   q      (N, 4) float32 orientation quaternions (w, x, y, z), e.g. the q.w..q.z columns of colvar-qorient;
 *   lags   nlags frame offsets d (1 <= d < N), HOST array in both forms;
 *   nchunk number of sub-chunks (>= 1); for lag d, chunk c covers samples [nb*c, min(N-d, nb*(c+1))), nb = ceil((N-d)/nchunk);
 *   out    (nlags, nchunk, 7) float64: sums over the chunk's samples of xx, yy, zz, xy, xz, yz of v = vec(dq), then the
 *          number of samples.  <v (x) v> = sums / count, <1 - 2|v|^2> = 1 - 2 (xx+yy+zz)/count; the whole-trajectory values
 *          are the sums over the chunks.  Products and sums in float64 on the float32 input. */
int sr_dq_moments_f32_dev(sr_ctx *, const float *q, int64_t N, const int32_t *lags_host, int nlags, int nchunk, double *out);
int sr_dq_moments_f32(sr_ctx *, const float *q, int64_t N, const int32_t *lags, int nlags, int nchunk, double *out);
/* the same on float64 quaternions: the reference's gmx-rotmat route (rotmatrix_to_quaternion, calculate-dq-distribution.py:
 * 482-497) keeps float64, and its short-lag moments (|v| ~ 1e-2) would lose five digits in a float32 round trip */
int sr_dq_moments_f64_dev(sr_ctx *, const double *q, int64_t N, const int32_t *lags_host, int nlags, int nchunk, double *out);
int sr_dq_moments_f64(sr_ctx *, const double *q, int64_t N, const int32_t *lags, int nlags, int nchunk, double *out);

/* ---- small device utilities ---------------------------------------------------------------
 * out[c*rows + r] = in[r*cols + c] (float64, device pointers): C(t) leaves kernel 1 as (lags, vectors)
 * like the reference, the fit reads (residues, lags). */
int sr_transpose_f64_dev(sr_ctx *, const double *in, int64_t rows, int64_t cols, double *out);
/* g matrices (rows, cols), contiguous one behind the other, each to (cols, rows) in ONE launch: the (lags, vectors) arrays of a group
 * of batches from the (g vectors, lags) rows sr_expfit_order_search_sums_f64_dev leaves.  Caller memory only, like the above.
 * Null pointer -2; g, rows or cols < 1, or more than 65535 matrices / 2 097 120 rows -3. */
int sr_transpose_batched_f64_dev(sr_ctx *, const double *in, int64_t g, int64_t rows, int64_t cols, double *out);

/* ---- host-side text I/O of the reference's xmgrace-style files (no device work) ----------------------------------
 * run-all.bash passes C(t) between its scripts as text: `<prefix>_Ctint.dat` is written by print_sxylist
 * (general_scripts.py:275-290) and read back by load_sxydylist (:182-213); `_fittedCt.dat` carries "%8g %8g" rows
 * (fitting_Ct_functions.py:107-126).  For 512 residues x 2 048 lags that is 31 + 38 MB of text per run, and with the kernels
 * at milliseconds its formatting / parsing in Python was 90 % of the chain's wall time.  These entry points produce exactly
 * the bytes / doubles of the Python code (numpy's array printer for the (C, dC) pairs, strtod for reading); a positive
 * return code (or `regular` = 0) means "not the regular case -- use the Python path" and nothing has been written.
 *   sr_text_write_sxydy_f64   legend_lines / xstr: nsets / npts strings separated by '\0'; ydy (nsets, npts, 2)
 *   sr_text_format_g8_pairs   n rows "%8g %8g\n" into out (>= 32 n bytes); returns the bytes written; offsets[k] = byte position
 *                             of row bounds[k] (optional: where the caller cuts the text into blocks)
 *   sr_text_open_sxydy        parse a file; info6 = {regular, nsets, npts, has_dy, legends, bytes of the '\0'-joined legends};
 *                             sr_text_sxydy_get copies x, y, dy (nsets, npts) and the legends out; sr_text_close_sxydy frees */
typedef struct sr_sxydy sr_sxydy;
int       sr_text_write_sxydy_f64(const char *path, const char *header, int64_t nsets, int64_t npts, const char *legend_lines,
                                  const char *xstr, const double *ydy, int nthreads);
int64_t   sr_text_format_g8_pairs(const double *a, const double *b, int64_t n, char *out, int64_t out_bytes, int nthreads,
                                  const int64_t *bounds, int64_t nb, int64_t *offsets);
sr_sxydy *sr_text_open_sxydy(const char *path, const char *key, int nthreads);
void      sr_text_close_sxydy(sr_sxydy *);
int       sr_text_sxydy_info(const sr_sxydy *, int64_t *info6);
int       sr_text_sxydy_get(const sr_sxydy *, double *x, double *y, double *dy, char *legends);

#ifdef __cplusplus
}
#endif
#endif /* SPINRELAX_HIP_H */
