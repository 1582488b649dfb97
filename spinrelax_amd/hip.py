"""
numpy-facing wrapper around the C ABI (spinrelax_amd/_lib.py -> libspinrelax_hip.so).

`Context` owns one sr_ctx (one GPU).  Methods without the `_dev` suffix take and return numpy arrays
(host buffers, blocking); `_dev` methods take raw device addresses (ints, e.g. torch
``tensor.data_ptr()``) and only enqueue work on the context's stream.
"""
import ctypes
import sys

import numpy as np

from . import _lib
from ._lib import SpinRelaxHipError, check


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _chunk_starts(chunk_start, R=None):
    """the chunk table as the C ABI takes it: None (regular chunks) or contiguous int64; with R, a table of another length raises"""
    if chunk_start is None:
        return None
    cs = np.ascontiguousarray(chunk_start, dtype=np.int64)
    if R is not None and cs.shape != (R,):
        raise ValueError('chunk_start must have R entries')
    return cs


def pair_columns(pairs, nV=None):
    """(nP, 2) vector indices -> the two contiguous int32 columns the C ABI takes; with nV, indices outside [0, nV) raise
    ValueError here (otherwise the library refuses them)"""
    pr = np.asarray(pairs)
    if pr.ndim != 2 or pr.shape[1] != 2 or pr.shape[0] < 1 or not np.issubdtype(pr.dtype, np.integer):
        raise ValueError('pairs must be an integer array of shape (nP, 2), nP >= 1')
    if nV is not None and (pr.min() < 0 or pr.max() >= nV):
        raise ValueError('pairs hold an index outside the %d vectors' % nV)
    return np.ascontiguousarray(pr[:, 0], dtype=np.int32), np.ascontiguousarray(pr[:, 1], dtype=np.int32)


def _windows(win_start, win_len):
    ws = np.ascontiguousarray(np.atleast_1d(win_start), dtype=np.int64)
    wl = np.ascontiguousarray(np.atleast_1d(win_len), dtype=np.int64)
    if ws.ndim != 1 or ws.shape != wl.shape:
        raise ValueError('win_start and win_len must be 1-D and of equal length')
    return ws, wl


def vechist_plan(N, nV, block_len=0):
    """How kernel 2 cuts a call of N frames and nV vectors into frame ranges (sr_vechist_plan: a host function, no Context and no
    GPU): dict(Fb, nB, m, sub, nranges).  Range rid < nB * m starts at frame (rid // m) * Fb + (rid % m) * sub and ends with its
    block, a later one (the frames behind the last full block) at nB * Fb + (rid - nB * m) * sub; ranges 4 k .. 4 k + 3 share a
    workgroup."""
    Fb, sub = ctypes.c_int64(), ctypes.c_int64()
    nB, m, nranges = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(_lib.load().sr_vechist_plan(int(N), int(nV), int(block_len or 0), ctypes.byref(Fb), ctypes.byref(nB), ctypes.byref(m),
                                      ctypes.byref(sub), ctypes.byref(nranges)), 'sr_vechist_plan')
    return dict(Fb=Fb.value, nB=nB.value, m=m.value, sub=sub.value, nranges=nranges.value)


def pack_reg_tiles(Npad, Vtot, v0, nV):
    """register tiles of kernel 0's production form for a shape, 0 when the shape takes the LDS tile (sr_pack_reg_tiles: a host
    function, no Context and no GPU)"""
    return int(_lib.load().sr_pack_reg_tiles(int(Npad), int(Vtot), int(v0), int(nV)))


def ct_pack_fused(formulation, F, series, tiles, aligned=True):
    """whether Context.ct_sums_pack_dev carries the pack inside the C(t) launch (sr_ct_pack_fused: a host function, no Context and
    no GPU)"""
    return bool(_lib.load().sr_ct_pack_fused(int(formulation), int(F), int(series), int(tiles), 1 if aligned else 0))


def symm_expm_plan(norm1, tau):
    """(s, products) of the scaling and squaring of exp(-R tau) for |R|_1 = norm1: s the least integer >= 0 with norm1 tau / 2^s <= 0.5,
    products = 11 + s (sr_symm_expm_plan: a host function, no Context and no GPU); SpinRelaxHipError for what symm_expm_dev refuses"""
    s, products = ctypes.c_int(), ctypes.c_int()
    check(_lib.load().sr_symm_expm_plan(float(norm1), float(tau), ctypes.byref(s), ctypes.byref(products)), 'sr_symm_expm_plan')
    return s.value, products.value


class Context:
    def __init__(self, device=0):
        self.lib = _lib.load()
        self.h = self.lib.sr_create(int(device))
        if not self.h:
            raise SpinRelaxHipError('sr_create(%d) failed: %s' % (device, _lib.last_error()))
        self.device = int(device)

    def close(self):
        """Deterministic teardown: synchronises the device and frees the context's work areas.  Call it (or use the
        context as a `with` block) before the interpreter exits; __del__ deliberately does NOT talk to HIP once the
        interpreter is finalising -- the runtime's own static destructors may already have run by then."""
        if getattr(self, 'h', None):
            self.lib.sr_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- plumbing ----
    def set_stream(self, stream_handle):
        check(self.lib.sr_set_stream(self.h, ctypes.c_void_p(stream_handle or 0)), 'sr_set_stream')

    def sync(self):
        check(self.lib.sr_sync(self.h), 'sr_sync')

    def set_option(self, name, value):
        check(self.lib.sr_set_option(self.h, name.encode(), int(value)), 'sr_set_option')
        if name in ('ct_cross_long_min_frames', 'ct_dipolar_long_min_frames', 'ct_dipolar_cross_long_min_frames'):
            setattr(self, name, int(value))           # the options that Python code acts on (ct.py's dispatch): keep what was accepted

    def stream_create(self, cu_mask_words=None, priority=0):
        """hipStream_t handle (int); cu_mask_words = iterable of 32-bit words, bit set = CU usable."""
        out = ctypes.c_void_p()
        if cu_mask_words is not None:
            words = (ctypes.c_uint32 * len(cu_mask_words))(*[int(w) & 0xFFFFFFFF for w in cu_mask_words])
            check(self.lib.sr_stream_create(self.h, words, len(cu_mask_words), priority, ctypes.byref(out)),
                  'sr_stream_create')
        else:
            check(self.lib.sr_stream_create(self.h, None, 0, priority, ctypes.byref(out)), 'sr_stream_create')
        return out.value

    def stream_destroy(self, handle):
        check(self.lib.sr_stream_destroy(self.h, ctypes.c_void_p(handle)), 'sr_stream_destroy')

    def device_sync(self):
        check(self.lib.sr_device_sync(self.h), 'sr_device_sync')

    def host_alloc(self, nbytes):
        """Page-locked host memory owned by the library (hipHostMalloc); returns the address."""
        p = self.lib.sr_host_alloc(self.h, int(nbytes))
        if not p:
            raise SpinRelaxHipError('sr_host_alloc(%d) failed: %s' % (nbytes, _lib.last_error()))
        return p

    def host_free(self, addr):
        check(self.lib.sr_host_free(self.h, ctypes.c_void_p(addr)), 'sr_host_free')

    def memcpy_d2h_async(self, host_addr, dev_ptr, nbytes):
        check(self.lib.sr_memcpy_d2h_async(self.h, ctypes.c_void_p(host_addr), ctypes.c_void_p(dev_ptr), int(nbytes)),
              'sr_memcpy_d2h_async')

    def memcpy_h2d_async(self, dev_ptr, host_addr, nbytes):
        check(self.lib.sr_memcpy_h2d_async(self.h, ctypes.c_void_p(dev_ptr), ctypes.c_void_p(host_addr), int(nbytes)),
              'sr_memcpy_h2d_async')

    def device_info(self):
        ncu = ctypes.c_int()
        hbm = ctypes.c_int64()
        lds = ctypes.c_int()
        name = ctypes.create_string_buffer(256)
        check(self.lib.sr_device_info(self.h, ctypes.byref(ncu), ctypes.byref(hbm), ctypes.byref(lds), name, 256),
              'sr_device_info')
        return dict(n_cu=ncu.value, hbm_bytes=hbm.value, lds_per_cu=lds.value, name=name.value.decode())

    def timer_start(self):
        check(self.lib.sr_timer_start(self.h), 'sr_timer_start')

    def timer_stop_ms(self):
        ms = ctypes.c_float()
        check(self.lib.sr_timer_stop_ms(self.h, ctypes.byref(ms)), 'sr_timer_stop_ms')
        return ms.value

    def max_frames_per_chunk(self):
        return int(self.lib.sr_ct_max_frames_per_chunk(self.h))

    # ---- kernel 1 ----
    def ct_palmer(self, vecs, R, F, v0=0, nV=None, chunk_start=None, mode=0):
        """vecs (N, Vtot, 3) float32 -> Ct, dCt (F//2, nV) float64.  calculate-Ct-from-traj.py:200-238."""
        vecs = _f32(vecs)
        if vecs.ndim != 3 or vecs.shape[2] != 3:
            raise ValueError('vecs must be (N, V, 3)')
        N, Vtot, _ = vecs.shape
        nV = Vtot - v0 if nV is None else nV
        L = F // 2
        Ct = np.empty((L, nV))
        dCt = np.empty((L, nV))
        cs = _chunk_starts(chunk_start, R)
        check(self.lib.sr_ct_palmer_f32(self.h, _ptr(vecs), N, Vtot, v0, nV, R, F, _ptr(cs), int(mode), _ptr(Ct), _ptr(dCt)),
              'sr_ct_palmer_f32')
        return Ct, dCt

    def pack_soa_dev(self, vecs_ptr, N, Vtot, v0, nV, soa_ptr, Npad):
        check(self.lib.sr_pack_soa_f32_dev(self.h, vecs_ptr, N, Vtot, v0, nV, soa_ptr, Npad), 'sr_pack_soa_f32_dev')

    def pack_soa_rot_dev(self, vecs_ptr, N, Vtot, v0, nV, quat_ptr, soa_ptr, Npad):
        check(self.lib.sr_pack_soa_rot_f32_dev(self.h, vecs_ptr, N, Vtot, v0, nV, quat_ptr, soa_ptr, Npad), 'sr_pack_soa_rot_f32_dev')

    def ct_palmer_dev(self, soa_ptr, Npad, R, F, nV, Ct_ptr, dCt_ptr, chunk_start=None, mode=0, psum_ptr=None):
        cs = _chunk_starts(chunk_start)
        check(self.lib.sr_ct_palmer_f32_dev(self.h, soa_ptr, Npad, R, F, nV, _ptr(cs), int(mode), psum_ptr, Ct_ptr, dCt_ptr),
              'sr_ct_palmer_f32_dev')

    def ct_sums_dev(self, soa_ptr, Npad, R, F, nV, psum_ptr, chunk_start=None, mode=0):
        cs = _chunk_starts(chunk_start)
        check(self.lib.sr_ct_palmer_sums_f32_dev(self.h, soa_ptr, Npad, R, F, nV, _ptr(cs), mode, psum_ptr),
              'sr_ct_palmer_sums_f32_dev')

    def ct_sums_pack_dev(self, soa_ptr, Npad, R, F, nV, psum_ptr, next_vecs_ptr, next_N, next_Vtot, next_v0, next_nV, next_soa_ptr,
                         next_Npad, chunk_start=None, mode=0):
        """ct_sums_dev, and pack_soa_dev of the next batch (another plane buffer) with it: one launch when the library can carry
        the pack inside the C(t) kernel (ct_pack_fused), else the pack in front of the C(t) kernel on the same stream"""
        cs = _chunk_starts(chunk_start)
        check(self.lib.sr_ct_palmer_sums_pack_f32_dev(self.h, soa_ptr, Npad, R, F, nV, _ptr(cs), mode, psum_ptr,
                                                      next_vecs_ptr, next_N, next_Vtot, next_v0, next_nV, next_soa_ptr, next_Npad),
              'sr_ct_palmer_sums_pack_f32_dev')

    def ct_sums_pack_plan(self, soa_ptr, Npad, R, F, nV, psum_ptr, next_vecs_ptr, next_N, next_Vtot, next_v0, next_nV, next_soa_ptr,
                          next_Npad, chunk_start=None, mode=0):
        """what ct_sums_pack_dev would do with these arguments, nothing queued: True = one launch carries the pack, False = the pack
        in front of the C(t) kernel; a refusal raises"""
        cs = _chunk_starts(chunk_start)
        rc = self.lib.sr_ct_palmer_sums_pack_plan(self.h, soa_ptr, Npad, R, F, nV, _ptr(cs), mode, psum_ptr,
                                                  next_vecs_ptr, next_N, next_Vtot, next_v0, next_nV, next_soa_ptr, next_Npad)
        if rc < 0:
            check(rc, 'sr_ct_palmer_sums_pack_plan')
        return rc == 1

    def ct_finalize_dev(self, psum_ptr, R, F, nV, Ct_ptr, dCt_ptr, CtT_ptr=None, dCtT_ptr=None):
        """mean / std over the chunks; with CtT_ptr / dCtT_ptr the same launch also writes the (nV, L) copies the fits read"""
        if CtT_ptr is None:
            check(self.lib.sr_ct_finalize_f64_dev(self.h, psum_ptr, R, F, nV, Ct_ptr, dCt_ptr), 'sr_ct_finalize_f64_dev')
        else:
            check(self.lib.sr_ct_finalize_t_f64_dev(self.h, psum_ptr, R, F, nV, Ct_ptr, dCt_ptr, CtT_ptr, dCtT_ptr),
                  'sr_ct_finalize_t_f64_dev')

    def psum_stride(self, F):
        return int(self.lib.sr_ct_psum_stride(F))

    # ---- pair cross-correlation functions (sr_ct_cross.hip) ----
    def ct_cross_max_frames(self):
        """longest chunk whose two series fit the LDS of a workgroup (sr_ct_cross_max_frames)"""
        return int(self.lib.sr_ct_cross_max_frames(self.h))

    def ct_cross_dev(self, soa_ptr, Npad, nV, R, F, pairs, P0_ptr, Ct_ptr, dCt_ptr, chunk_start=None, sym=1, mode=0, psum_ptr=None,
                     dP0_ptr=None):
        """P0 (nP) (and its error dP0 when dP0_ptr is given), C(t) and dC(t) (F//2, nP) of the pairs (nP, 2) from packed planes into
        device arrays (sr_ct_cross_f32_dev); asynchronous on the context's stream"""
        self._pairs_dev('sr_ct_cross_f32_dev', soa_ptr, Npad, nV, R, F, pairs, chunk_start, sym, mode, psum_ptr, P0_ptr, dP0_ptr, Ct_ptr, dCt_ptr)

    def _pairs_dev(self, name, planes_ptr, Npad, nV, R, F, pairs, chunk_start, sym, mode, psum_ptr, *out_ptrs):
        """a pair entry point of the library by name: staged or blocked, unit-vector planes or the dipolar pack (whose wsum2 follows dCt)"""
        pi, pj = pair_columns(pairs)
        cs = _chunk_starts(chunk_start)
        check(getattr(self.lib, name)(self.h, planes_ptr, int(Npad), int(nV), int(R), int(F), _ptr(cs), _ptr(pi), _ptr(pj), pi.size, int(sym),
                                      int(mode), psum_ptr, *out_ptrs), name)

    def _dipolar_dev(self, name, planes_ptr, Npad, nV, R, F, chunk_start, mode, psum_ptr, Ct_ptr, dCt_ptr, wmean_ptr):
        """sr_ct_dipolar_f32_dev or its blocked counterpart, by name"""
        cs = _chunk_starts(chunk_start)
        check(getattr(self.lib, name)(self.h, planes_ptr, int(Npad), int(nV), int(R), int(F), _ptr(cs), int(mode), psum_ptr, Ct_ptr, dCt_ptr,
                                      wmean_ptr), name)

    ct_cross_long_min_frames = 6625     # the library's default of the option: the first length ct_cross refuses

    def ct_cross_long_max_frames(self):
        """longest chunk the blocked form of the pair cross-correlation takes (sr_ct_cross_long_max_frames)"""
        return int(self.lib.sr_ct_cross_long_max_frames(self.h))

    def ct_cross_long_dev(self, soa_ptr, Npad, nV, R, F, pairs, P0_ptr, Ct_ptr, dCt_ptr, chunk_start=None, sym=1, mode=0, psum_ptr=None,
                          dP0_ptr=None):
        """ct_cross_dev for chunks of 5462 .. ct_cross_long_max_frames() frames, by blocked transforms (sr_ct_cross_long_f32_dev)"""
        self._pairs_dev('sr_ct_cross_long_f32_dev', soa_ptr, Npad, nV, R, F, pairs, chunk_start, sym, mode, psum_ptr, P0_ptr, dP0_ptr, Ct_ptr,
                        dCt_ptr)

    # ---- distance-weighted dipolar correlation function (sr_ct_dipolar.hip) ----
    def ct_dipolar_max_frames(self):
        """longest chunk whose four series a_x, a_y, a_z, w fit the LDS of a workgroup (sr_ct_dipolar_max_frames)"""
        return int(self.lib.sr_ct_dipolar_max_frames(self.h))

    def pack_dipolar_dev(self, vecs_ptr, dist_ptr, N, Vtot, v0, nV, planes_ptr, Npad, rref_ptr):
        """frame-major vectors (N, Vtot, 3) float32 of any length (and, when dist_ptr is not None, distances (N, Vtot) float32 that
        replace their lengths) -> planes (nV, 4, Npad) float32 a_x, a_y, a_z, w and r_ref (nV) float64 (sr_pack_dipolar_f32_dev);
        asynchronous on the context's stream"""
        check(self.lib.sr_pack_dipolar_f32_dev(self.h, vecs_ptr, dist_ptr, int(N), int(Vtot), int(v0), int(nV), planes_ptr, int(Npad), rref_ptr),
              'sr_pack_dipolar_f32_dev')

    def ct_dipolar_dev(self, planes_ptr, Npad, nV, R, F, Ct_ptr, dCt_ptr, wmean_ptr, chunk_start=None, mode=0, psum_ptr=None):
        """C_dd(t) and dC_dd(t) (F//2, nV) and wmean (nV, 2) = <w>, <w^2> from the four planes of pack_dipolar_dev into device arrays
        (sr_ct_dipolar_f32_dev); asynchronous on the context's stream"""
        self._dipolar_dev('sr_ct_dipolar_f32_dev', planes_ptr, Npad, nV, R, F, chunk_start, mode, psum_ptr, Ct_ptr, dCt_ptr, wmean_ptr)

    # ---- bond-vector correlation function split into the five tumbling modes (sr_ct_modes.hip) ----
    def ct_modes_max_frames(self):
        """longest chunk whose five signal series fit the LDS of a workgroup (sr_ct_modes_max_frames)"""
        return int(self.lib.sr_ct_modes_max_frames(self.h))

    def pack_modes_dev(self, vecs_ptr, N, Vtot, v0, nV, planes_ptr, Npad, bad_ptr, frame=None):
        """frame-major vectors (N, Vtot, 3) float32 of any positive length -> planes (nV, 5, Npad) float32 of the five signals
        u_z^2 - 1/3, u_x^2 - u_y^2, u_y u_z, u_x u_z, u_x u_y of u = R(frame) v / |v| and bad (nV) int32, 1 for a vector with a frame that
        is not finite or of zero length (sr_pack_modes_f32_dev); frame: a unit quaternion (w, x, y, z) or None; asynchronous on the
        context's stream"""
        fq = self._frame(frame)
        check(self.lib.sr_pack_modes_f32_dev(self.h, vecs_ptr, int(N), int(Vtot), int(v0), int(nV), _ptr(fq), planes_ptr, int(Npad), bad_ptr),
              'sr_pack_modes_f32_dev')

    def ct_modes_dev(self, planes_ptr, Npad, nV, R, F, H_ptr, dH_ptr, smean_ptr, chunk_start=None, mode=0, psum_ptr=None):
        """the six mode sums H and dH (F//2 + 1, nV, 6), lag 0 first, and smean (nV, 5), the means of the five signals, from the planes of
        pack_modes_dev into device arrays (sr_ct_modes_f32_dev); asynchronous on the context's stream"""
        cs = _chunk_starts(chunk_start)
        check(self.lib.sr_ct_modes_f32_dev(self.h, planes_ptr, int(Npad), int(nV), int(R), int(F), _ptr(cs), int(mode), psum_ptr, H_ptr, dH_ptr,
                                           smean_ptr), 'sr_ct_modes_f32_dev')

    # ---- distance-weighted pair cross-correlation functions (sr_ct_dipolar_cross.hip) ----
    def ct_dipolar_cross_max_frames(self):
        """longest chunk whose eight series (a_x, a_y, a_z, w of both vectors of a pair) fit the LDS of a workgroup
        (sr_ct_dipolar_cross_max_frames)"""
        return int(self.lib.sr_ct_dipolar_cross_max_frames(self.h))

    def ct_dipolar_cross_dev(self, planes_ptr, Npad, nV, R, F, pairs, P0_ptr, Ct_ptr, dCt_ptr, wsum2_ptr, chunk_start=None, sym=1, mode=0,
                             psum_ptr=None, dP0_ptr=None):
        """P0 (nP) (and its error dP0 when dP0_ptr is given), C(t) and dC(t) (F//2, nP) of the pairs (nP, 2) and wsum2 (nP, R, 2), the sums
        of w_i^2 and w_j^2 over every chunk, from the four planes of pack_dipolar_dev into device arrays (sr_ct_dipolar_cross_f32_dev);
        asynchronous on the context's stream"""
        self._pairs_dev('sr_ct_dipolar_cross_f32_dev', planes_ptr, Npad, nV, R, F, pairs, chunk_start, sym, mode, psum_ptr, P0_ptr, dP0_ptr, Ct_ptr,
                        dCt_ptr, wsum2_ptr)

    # ---- both for long chunks: blocked transforms (sr_ct_dipolar_long.hip) ----
    ct_dipolar_long_min_frames = 10017          # the library's defaults of the two options: the first lengths that ct_dipolar and
    ct_dipolar_cross_long_min_frames = 4897     # ct_dipolar_cross refuse

    def ct_dipolar_long_max_frames(self):
        """longest chunk the blocked form of the dipolar correlation function takes (sr_ct_dipolar_long_max_frames)"""
        return int(self.lib.sr_ct_dipolar_long_max_frames(self.h))

    def ct_dipolar_cross_long_max_frames(self):
        """longest chunk the blocked form of the dipolar pair cross-correlation takes (sr_ct_dipolar_cross_long_max_frames)"""
        return int(self.lib.sr_ct_dipolar_cross_long_max_frames(self.h))

    def ct_dipolar_long_dev(self, planes_ptr, Npad, nV, R, F, Ct_ptr, dCt_ptr, wmean_ptr, chunk_start=None, mode=0, psum_ptr=None):
        """ct_dipolar_dev for chunks of 5462 .. ct_dipolar_long_max_frames() frames, by blocked transforms (sr_ct_dipolar_long_f32_dev); the
        planes must come from pack_dipolar_dev"""
        self._dipolar_dev('sr_ct_dipolar_long_f32_dev', planes_ptr, Npad, nV, R, F, chunk_start, mode, psum_ptr, Ct_ptr, dCt_ptr, wmean_ptr)

    def ct_dipolar_cross_long_dev(self, planes_ptr, Npad, nV, R, F, pairs, P0_ptr, Ct_ptr, dCt_ptr, wsum2_ptr, chunk_start=None, sym=1, mode=0,
                                  psum_ptr=None, dP0_ptr=None):
        """ct_dipolar_cross_dev for chunks of 4097 .. ct_dipolar_cross_long_max_frames() frames, by blocked transforms
        (sr_ct_dipolar_cross_long_f32_dev); the planes must come from pack_dipolar_dev"""
        self._pairs_dev('sr_ct_dipolar_cross_long_f32_dev', planes_ptr, Npad, nV, R, F, pairs, chunk_start, sym, mode, psum_ptr, P0_ptr, dP0_ptr,
                        Ct_ptr, dCt_ptr, wsum2_ptr)

    # ---- iRED matrix (sr_ired.hip) ----
    def ired_matrix_dev(self, soa_ptr, Npad, nV, win_start, win_len, M_ptr):
        """M[w] = mean over frames [win_start[w], win_start[w] + win_len[w]) of P2(u_i . u_j) from packed planes, into the device
        array M_ptr (W, nV, nV) float64 (sr_ired_matrix_f32_dev); asynchronous on the context's stream"""
        ws, wl = _windows(win_start, win_len)
        check(self.lib.sr_ired_matrix_f32_dev(self.h, soa_ptr, int(Npad), int(nV), _ptr(ws), _ptr(wl), ws.size, M_ptr),
              'sr_ired_matrix_f32_dev')

    # ---- iRED mode correlation functions (sr_ired_modes.hip) ----
    def ired_mode_ct_dev(self, soa_ptr, Npad, nV, win_start, win_len, coef_ptr, K, n_lags, Cm_ptr):
        """C_m(k), k < n_lags, of the K rows of every window's coefficient matrix (device array coef_ptr (W, K, nV) float64) from
        packed planes, into the device array Cm_ptr (W, K, n_lags) float64 (sr_ired_mode_ct_f32_dev); asynchronous on the
        context's stream"""
        ws, wl = _windows(win_start, win_len)
        check(self.lib.sr_ired_mode_ct_f32_dev(self.h, soa_ptr, int(Npad), int(nV), _ptr(ws), _ptr(wl), ws.size, coef_ptr, int(K),
                                               int(n_lags), Cm_ptr), 'sr_ired_mode_ct_f32_dev')

    # ---- all-pairs dipolar map, at chosen lags, split into tumbling modes (sr_noe.hip) ----
    @staticmethod
    def _lags(lags):
        lg = np.ascontiguousarray(np.atleast_1d(lags))
        if lg.size == 0:                                   # an empty list is the library's to refuse
            lg = lg.astype(np.int32)
        if lg.ndim != 1 or lg.dtype.kind not in 'iu':
            raise ValueError('lags must be a 1-D list of integers')
        if lg.size and (lg.min() < -2 ** 31 or lg.max() >= 2 ** 31):
            raise ValueError('lags must fit 32 bits')
        return np.ascontiguousarray(lg, dtype=np.int32)

    @staticmethod
    def _frame(frame):
        if frame is None:
            return None
        fq = _f64(frame)
        if fq.shape != (4,):
            raise ValueError('frame must be a quaternion (w, x, y, z)')
        return fq

    @staticmethod
    def _noe_index(index):
        idx = np.ascontiguousarray(index, dtype=np.int32)
        if idx.ndim != 1:
            raise ValueError('index must be 1-D')
        return idx

    @classmethod
    def _noe_host(cls, xyz, index, quat, block_start, block_len):
        """the host arrays of a noe_* call as the library takes them: xyz (frames, atoms, 3) float32, index 1-D int32, quat (frames, 4)
        float64 or None, the block table int64 (without one: one block of all frames)"""
        xyz = _f32(xyz)
        if xyz.ndim != 3 or xyz.shape[2] != 3:
            raise ValueError('xyz must be (frames, atoms, 3)')
        idx = cls._noe_index(index)
        qq = None if quat is None else _f64(quat)
        if qq is not None and qq.shape != (xyz.shape[0], 4):
            raise ValueError('quat must be (frames, 4)')
        if block_start is None:
            block_start, block_len = [0], [xyz.shape[0]]
        return (xyz, idx, qq) + _windows(block_start, block_len)

    def noe_pairs_dev(self, xyz_ptr, nFrames, nAtoms, index, quat_ptr, block_start, block_len, sums_ptr, mode=0):
        """Block sums of r^-6 and d'_a d'_b r^-5 (xx, yy, zz, xy, xz, yz) of every pair i < j of the atoms `index` from the device
        coordinates xyz_ptr (nFrames, nAtoms, 3) float32, d' = d rotated by the frame's unit quaternion of the device array quat_ptr
        (nFrames, 4) float64 (None: identity), into the device array sums_ptr (B, P (P - 1) / 2, 7) float64, pairs in the order of
        noe.pair_index (sr_noe_pairs_f32_dev); asynchronous on the context's stream"""
        idx, (bs, bl) = self._noe_index(index), _windows(block_start, block_len)
        check(self.lib.sr_noe_pairs_f32_dev(self.h, xyz_ptr, int(nFrames), int(nAtoms), _ptr(idx), idx.size, quat_ptr, _ptr(bs), _ptr(bl),
                                            bs.size, int(mode), sums_ptr), 'sr_noe_pairs_f32_dev')

    def noe_pairs(self, xyz, index, quat=None, block_start=None, block_len=None, mode=0):
        """The same of host arrays: xyz (nFrames, nAtoms, 3) float32, quat (nFrames, 4) float64 or None -> sums (B, P (P - 1) / 2, 7)
        float64; without block tables one block of all frames (sr_noe_pairs_f32)"""
        xyz, idx, qq, bs, bl = self._noe_host(xyz, index, quat, block_start, block_len)
        nF, nA, P = xyz.shape[0], xyz.shape[1], idx.size
        self.noe_pairs_check(nF, nA, idx, bs, bl, mode)      # a map beyond the device's memory is refused before its host array exists
        sums = np.empty((bs.size, P * (P - 1) // 2, 7))
        check(self.lib.sr_noe_pairs_f32(self.h, _ptr(xyz), nF, nA, _ptr(idx), P, _ptr(qq), _ptr(bs), _ptr(bl), bs.size, int(mode),
                                        _ptr(sums)), 'sr_noe_pairs_f32')
        return sums

    def noe_pairs_check(self, nFrames, nAtoms, index, block_start, block_len, mode=0):
        """raises what noe_pairs / noe_pairs_dev would refuse (-3) for these arguments, the size of the result included; allocates and
        queues nothing (sr_noe_pairs_check)"""
        idx, (bs, bl) = self._noe_index(index), _windows(block_start, block_len)
        check(self.lib.sr_noe_pairs_check(self.h, int(nFrames), int(nAtoms), _ptr(idx), idx.size, _ptr(bs), _ptr(bl), bs.size, int(mode)),
              'sr_noe_pairs_check')

    def noe_tile(self):
        """atoms per tile side of k_noe_pairs"""
        return int(self.lib.sr_noe_tile())

    def noe_frame_batch(self):
        """frames per LDS stage of k_noe_pairs"""
        return int(self.lib.sr_noe_frame_batch())

    # the dipolar map at chosen lags
    def noe_lagged_dev(self, xyz_ptr, nFrames, nAtoms, index, quat_ptr, block_start, block_len, lags, G_ptr, mode=0):
        """G[b][q][pair] = sum over the origins t of block b of [1.5 cos^2 - 0.5] r(t)^-3 r(t + k)^-3 at the lags k = lags[q] (strictly
        increasing, >= 0, below the shortest block; at most 64), cos the angle between d'(t) and d'(t + k), of every pair i < j of the
        atoms `index` from the device coordinates xyz_ptr (nFrames, nAtoms, 3) float32 and the device quaternions quat_ptr (nFrames,
        4) float64 (None: identity), into the device array G_ptr (B, K, P (P - 1) / 2) float64, pairs in the order of noe.pair_index
        (sr_noe_lagged_f32_dev); asynchronous on the context's stream"""
        idx, (bs, bl) = self._noe_index(index), _windows(block_start, block_len)
        lg = self._lags(lags)
        check(self.lib.sr_noe_lagged_f32_dev(self.h, xyz_ptr, int(nFrames), int(nAtoms), _ptr(idx), idx.size, quat_ptr, _ptr(bs), _ptr(bl),
                                             bs.size, _ptr(lg), lg.size, int(mode), G_ptr), 'sr_noe_lagged_f32_dev')

    def noe_lagged(self, xyz, index, lags, quat=None, block_start=None, block_len=None, mode=0):
        """The same of host arrays: xyz (nFrames, nAtoms, 3) float32, quat (nFrames, 4) float64 or None -> G (B, K, P (P - 1) / 2)
        float64; without block tables one block of all frames (sr_noe_lagged_f32)"""
        xyz, idx, qq, bs, bl = self._noe_host(xyz, index, quat, block_start, block_len)
        lg = self._lags(lags)
        nF, nA, P = xyz.shape[0], xyz.shape[1], idx.size
        self.noe_lagged_check(nF, nA, idx, bs, bl, lg, mode)    # a result beyond the device's memory is refused before its host array exists
        G = np.empty((bs.size, lg.size, P * (P - 1) // 2))
        check(self.lib.sr_noe_lagged_f32(self.h, _ptr(xyz), nF, nA, _ptr(idx), P, _ptr(qq), _ptr(bs), _ptr(bl), bs.size, _ptr(lg), lg.size,
                                         int(mode), _ptr(G)), 'sr_noe_lagged_f32')
        return G

    def noe_lagged_check(self, nFrames, nAtoms, index, block_start, block_len, lags, mode=0):
        """raises what noe_lagged / noe_lagged_dev would refuse (-3) for these arguments, the size of the result included; allocates and
        queues nothing (sr_noe_lagged_check)"""
        idx, (bs, bl) = self._noe_index(index), _windows(block_start, block_len)
        lg = self._lags(lags)
        check(self.lib.sr_noe_lagged_check(self.h, int(nFrames), int(nAtoms), _ptr(idx), idx.size, _ptr(bs), _ptr(bl), bs.size, _ptr(lg), lg.size,
                                           int(mode)), 'sr_noe_lagged_check')

    def noe_lagged_splits(self, P, longest_block, B=1):
        """frame splits S of a lagged map of P atoms over B blocks, the longest of longest_block frames: the map's own rule, whatever
        the lags"""
        return int(self.lib.sr_noe_lagged_splits(int(P), int(longest_block), int(B)))

    # the lagged map split into the tumbling modes of an anisotropic tensor
    def noe_modes_dev(self, xyz_ptr, nFrames, nAtoms, index, quat_ptr, block_start, block_len, lags, H_ptr, frame=None, mode=0):
        """H[b][q][pair][0 .. 5]: the six mode sums of k_noe_modes (sr_noe.hip: qz qz', dl dl', sym qz dl', yz yz', xz xz', xy xy', each
        weighted with r(t)^-3 r(t + k)^-3) over the origins t of block b at the lags k = lags[q], of every pair i < j of the atoms `index`,
        the pair vectors taken into the frame R(frame) R(quat[t]): frame a unit quaternion (w, x, y, z) on the host, None: identity;
        quat_ptr the device quaternions (nFrames, 4) float64, None: identity.  Into the device array H_ptr (B, K, P (P - 1) / 2, 6)
        float64 (sr_noe_modes_f32_dev); asynchronous on the context's stream"""
        idx, (bs, bl) = self._noe_index(index), _windows(block_start, block_len)
        lg, fq = self._lags(lags), self._frame(frame)
        check(self.lib.sr_noe_modes_f32_dev(self.h, xyz_ptr, int(nFrames), int(nAtoms), _ptr(idx), idx.size, quat_ptr, _ptr(fq), _ptr(bs),
                                            _ptr(bl), bs.size, _ptr(lg), lg.size, int(mode), H_ptr), 'sr_noe_modes_f32_dev')

    def noe_modes(self, xyz, index, lags, quat=None, frame=None, block_start=None, block_len=None, mode=0):
        """The same of host arrays: xyz (nFrames, nAtoms, 3) float32, quat (nFrames, 4) float64 or None -> H (B, K, P (P - 1) / 2, 6)
        float64; without block tables one block of all frames (sr_noe_modes_f32)"""
        xyz, idx, qq, bs, bl = self._noe_host(xyz, index, quat, block_start, block_len)
        lg, fq = self._lags(lags), self._frame(frame)
        nF, nA, P = xyz.shape[0], xyz.shape[1], idx.size
        self.noe_modes_check(nF, nA, idx, bs, bl, lg, frame=fq, mode=mode)   # a result beyond the device's memory is refused before its host array exists
        H = np.empty((bs.size, lg.size, P * (P - 1) // 2, 6))
        check(self.lib.sr_noe_modes_f32(self.h, _ptr(xyz), nF, nA, _ptr(idx), P, _ptr(qq), _ptr(fq), _ptr(bs), _ptr(bl), bs.size, _ptr(lg),
                                        lg.size, int(mode), _ptr(H)), 'sr_noe_modes_f32')
        return H

    def noe_modes_check(self, nFrames, nAtoms, index, block_start, block_len, lags, frame=None, mode=0):
        """raises what noe_modes / noe_modes_dev would refuse (-3) for these arguments, the size of the result and the frame quaternion
        included; allocates and queues nothing (sr_noe_modes_check)"""
        idx, (bs, bl) = self._noe_index(index), _windows(block_start, block_len)
        lg, fq = self._lags(lags), self._frame(frame)
        check(self.lib.sr_noe_modes_check(self.h, int(nFrames), int(nAtoms), _ptr(idx), idx.size, _ptr(bs), _ptr(bl), bs.size, _ptr(lg), lg.size,
                                          _ptr(fq), int(mode)), 'sr_noe_modes_check')

    # ---- NOESY from the dipolar map (sr_noesy.hip) ----
    @staticmethod
    def _noesy_modes_args(a, c, E, P, tau_e, leak):
        a, c, E = _f64(a), _f64(c), _f64(E)
        P = int(P)
        npairs = P * (P - 1) // 2
        if a.shape != (npairs, 5) or c.shape != (npairs, 5) or E.shape != (5,):
            raise ValueError('a and c must be (P (P - 1) / 2, 5) = (%d, 5) for P = %d spins and E (5)' % (npairs, P))
        tp_arr = tm_arr = lk_arr = None
        te = lk = 0.0
        if np.ndim(tau_e) == 0:
            te = float(tau_e)
        else:
            t = _f64(tau_e)
            if t.shape == (npairs,):
                tp_arr = t
            elif t.shape == (npairs, 5):
                tm_arr = t
            else:
                raise ValueError('tau_e must be a scalar, one value per pair or one per pair and mode')
        if np.ndim(leak) == 0:
            lk = float(leak)
        else:
            lk_arr = _f64(leak)
            if lk_arr.shape != (P,):
                raise ValueError('leak must be a scalar or one value per spin')
        return a, c, E, P, tp_arr, tm_arr, lk_arr, te, lk

    def noesy_rates_modes_dev(self, a, c, E, P, omega_H, tau_e, leak, prefactor, R_ptr):
        """The relaxation matrix of P spins under anisotropic tumbling from the host arrays a, c (P (P - 1) / 2, 5), the mode amplitudes
        at lag 0 and their plateaus in units of <r^-6> (noe.mode_amplitudes, noe.mode_plateau), and the tensor's five rates E (1 / s):
        J(w) = sum_m [c_m g(E_m, w) + max(a_m - c_m, 0) g(E_m + 1 / tau_e, w)], R_ij = prefactor [6 J(2 omega_H) - J(0)],
        R_ii = sum_j prefactor [J(0) + 3 J(omega_H) + 6 J(2 omega_H)] + leak_i, into the device array R_ptr (P, P) float64; tau_e a
        scalar, one per pair or one per pair and mode, leak a scalar or one per spin (sr_noesy_rates_modes_f64_dev); returns when the
        host arrays are consumed"""
        a, c, E, P, tp, tm, lk_arr, te, lk = self._noesy_modes_args(a, c, E, P, tau_e, leak)
        check(self.lib.sr_noesy_rates_modes_f64_dev(self.h, _ptr(a), _ptr(c), _ptr(E), _ptr(tp), _ptr(tm), _ptr(lk_arr), P, float(omega_H), te, lk,
                                                    float(prefactor), R_ptr), 'sr_noesy_rates_modes_f64_dev')

    def noesy_rates_modes(self, a, c, E, P, omega_H, tau_e, leak, prefactor):
        """The same with the result on the host: R (P, P) float64 (sr_noesy_rates_modes_f64)"""
        a, c, E, P, tp, tm, lk_arr, te, lk = self._noesy_modes_args(a, c, E, P, tau_e, leak)
        R = np.empty((max(P, 0), max(P, 0)))
        check(self.lib.sr_noesy_rates_modes_f64(self.h, _ptr(a), _ptr(c), _ptr(E), _ptr(tp), _ptr(tm), _ptr(lk_arr), P, float(omega_H), te, lk,
                                                float(prefactor), _ptr(R)), 'sr_noesy_rates_modes_f64')
        return R

    @staticmethod
    def _noesy_args(A6, S2, P, tau_e, leak):
        A6, S2 = _f64(A6), _f64(S2)
        P = int(P)
        npairs = P * (P - 1) // 2
        if A6.shape != (npairs,) or S2.shape != (npairs,):
            raise ValueError('A6 and S2 must hold the P (P - 1) / 2 = %d pairs of P = %d spins' % (npairs, P))
        te_arr = lk_arr = None
        te = lk = 0.0
        if np.ndim(tau_e) == 0:
            te = float(tau_e)
        else:
            te_arr = _f64(tau_e)
            if te_arr.shape != (npairs,):
                raise ValueError('tau_e must be a scalar or one value per pair')
        if np.ndim(leak) == 0:
            lk = float(leak)
        else:
            lk_arr = _f64(leak)
            if lk_arr.shape != (P,):
                raise ValueError('leak must be a scalar or one value per spin')
        return A6, S2, P, te_arr, lk_arr, te, lk

    def noesy_rates_dev(self, A6, S2, P, omega_H, tau_c, tau_e, leak, prefactor, R_ptr):
        """The relaxation matrix of P spins from the map's host arrays A6 = <r^-6> and S2 (P (P - 1) / 2 each, pairs in the order of
        noe.pair_index): R_ij = sigma_ij = prefactor A6 [6 J(2 omega_H) - J(0)], R_ii = sum_j prefactor A6 [J(0) + 3 J(omega_H) +
        6 J(2 omega_H)] + leak_i with the model-free J of tau_c, S2 and tau_e, into the device array R_ptr (P, P) float64; tau_e a
        scalar or one per pair, leak a scalar or one per spin (sr_noesy_rates_f64_dev); returns when the host arrays are consumed"""
        A6, S2, P, te_arr, lk_arr, te, lk = self._noesy_args(A6, S2, P, tau_e, leak)
        check(self.lib.sr_noesy_rates_f64_dev(self.h, _ptr(A6), _ptr(S2), _ptr(te_arr), _ptr(lk_arr), P, float(omega_H), float(tau_c), te, lk,
                                              float(prefactor), R_ptr), 'sr_noesy_rates_f64_dev')

    def noesy_rates(self, A6, S2, P, omega_H, tau_c, tau_e, leak, prefactor):
        """The same with the result on the host: R (P, P) float64 (sr_noesy_rates_f64)"""
        A6, S2, P, te_arr, lk_arr, te, lk = self._noesy_args(A6, S2, P, tau_e, leak)
        R = np.empty((max(P, 0), max(P, 0)))
        check(self.lib.sr_noesy_rates_f64(self.h, _ptr(A6), _ptr(S2), _ptr(te_arr), _ptr(lk_arr), P, float(omega_H), float(tau_c), te, lk,
                                          float(prefactor), _ptr(R)), 'sr_noesy_rates_f64')
        return R

    def symm_mul_dev(self, A_ptr, B_ptr, P, C_ptr, alpha=1.0, beta=0.0):
        """C = alpha A B + beta I of the symmetric device matrices A_ptr and B_ptr (P, P) float64 that commute, into the device array
        C_ptr, which may be either of them; for symmetric matrices that do not commute the 64 x 64 tiles with tile row <= tile column
        of that expression (of a diagonal tile i <= j), mirrored below (sr_symm_mul_f64_dev); asynchronous on the context's stream"""
        check(self.lib.sr_symm_mul_f64_dev(self.h, A_ptr, B_ptr, int(P), float(alpha), float(beta), C_ptr), 'sr_symm_mul_f64_dev')

    def symm_expm_dev(self, R_ptr, P, mixing_times, out_ptr):
        """out[k] = exp(-R tau_k) of the symmetric device matrix R_ptr (P, P) float64 for the host list mixing_times, into the device
        array out_ptr (n_tau, P, P) float64, each from R on its own by scaling and squaring (sr_symm_expm_f64_dev); waits for
        |R|_1, then asynchronous on the context's stream"""
        tau = np.ascontiguousarray(np.atleast_1d(mixing_times), dtype=np.float64)
        if tau.ndim != 1:
            raise ValueError('mixing_times must be 1-D')
        check(self.lib.sr_symm_expm_f64_dev(self.h, R_ptr, int(P), _ptr(tau), tau.size, out_ptr), 'sr_symm_expm_f64_dev')

    symm_expm_plan = staticmethod(symm_expm_plan)

    def symm_expm_check(self, P, n_tau):
        """raises what symm_expm_dev would refuse (-3) for these sizes, with the results counted against the free device memory too;
        allocates and queues nothing (sr_symm_expm_check)"""
        check(self.lib.sr_symm_expm_check(self.h, int(P), int(n_tau)), 'sr_symm_expm_check')

    def xh_quat_dev(self, xyz_ptr, nFrames, nAtoms, fit_indices, ref_xyz, quat_ptr):
        """The front end's superposition alone: the unit quaternions (w, x, y, z) that rotate every frame of the device coordinates
        onto ref_xyz over fit_indices, into the device array quat_ptr (nFrames, 4) float64 (sr_xh_vectors_f32_dev with no vector
        output); asynchronous on the context's stream"""
        fi = np.ascontiguousarray(fit_indices, dtype=np.int32)
        rx = _f32(ref_xyz)
        if rx.shape != (nAtoms, 3):
            raise ValueError('ref_xyz must be (atoms, 3)')
        bond = np.zeros(1, dtype=np.int32)              # the entry point wants one bond; none is written
        check(self.lib.sr_xh_vectors_f32_dev(self.h, xyz_ptr, int(nFrames), int(nAtoms), _ptr(bond), _ptr(bond), 1, _ptr(fi), fi.size,
                                             _ptr(rx), None, None, quat_ptr), 'sr_xh_vectors_f32_dev')

    # ---- resident vectors (sr_vectors.hip) ----
    def vectors(self, nV, capacity=0):
        """An empty ResidentVectors object for nV vectors (this rank's columns)."""
        return ResidentVectors(self, nV, capacity)

    def counter(self, name):
        v = ctypes.c_uint64()
        check(self.lib.sr_counter(self.h, name.encode(), ctypes.byref(v)), 'sr_counter')
        return int(v.value)

    def ct_finalize_sums(self, sums, F):
        """mean / std over the replicates from raw sums (nV, R, F//2): Ct, dCt (F//2, nV) -- the kernel of a single-process run"""
        sums = _f64(sums)
        nV, R, L = sums.shape
        if L != F // 2:
            raise ValueError('sums must be (vectors, chunks, F//2)')
        Ct = np.empty((L, nV))
        dCt = np.empty((L, nV))
        check(self.lib.sr_ct_finalize_sums_f64(self.h, _ptr(sums), R, int(F), nV, _ptr(Ct), _ptr(dCt)), 'sr_ct_finalize_sums_f64')
        return Ct, dCt

    # ---- kernel 2 ----
    def rotate_hist(self, vecs, q, edges_phi, edges_cos, v0=0, nV=None, block_len=0, want_outer=True):
        """vecs (N, Vtot, 3) float32 -> hist (nV, nphi, ncos), vecsum (nV,3), outer (nB, nV, 6).  The edges must be
        numpy.linspace(-pi, pi, nphi + 1) and numpy.linspace(-1, 1, ncos + 1); any others are refused."""
        vecs = _f32(vecs)
        N, Vtot, _ = vecs.shape
        nV = Vtot - v0 if nV is None else nV
        ep = _f64(edges_phi)
        ec = _f64(edges_cos)
        nphi, ncos = ep.size - 1, ec.size - 1
        qq = None if q is None else _f64(q)
        hist = np.empty((nV, nphi, ncos))
        vecsum = np.empty((nV, 3))
        Fb = block_len if (block_len and 0 < block_len <= N) else N
        nB = N // Fb
        outer = np.empty((nB, nV, 6)) if want_outer else None
        check(self.lib.sr_rotate_hist_f32(self.h, _ptr(vecs), N, Vtot, v0, nV, _ptr(qq), _ptr(ep), nphi, _ptr(ec), ncos,
                                          _ptr(hist), _ptr(vecsum), _ptr(outer), int(block_len or 0)), 'sr_rotate_hist_f32')
        return hist, vecsum, outer

    def rotate_hist_dev(self, soa_ptr, Npad, N, nV, q, edges_phi, edges_cos, hist_ptr, vecsum_ptr, outer_ptr, block_len):
        ep = _f64(edges_phi)
        ec = _f64(edges_cos)
        qq = None if q is None else _f64(q)
        check(self.lib.sr_rotate_hist_f32_dev(self.h, soa_ptr, Npad, N, nV, _ptr(qq), _ptr(ep), ep.size - 1, _ptr(ec),
                                              ec.size - 1, hist_ptr, vecsum_ptr, outer_ptr, int(block_len or 0)),
              'sr_rotate_hist_f32_dev')

    def rotate_vectors(self, vecs, q, v0=0, nV=None):
        """q: (4,) one rotation for everything, or (N, 4) one UNIT quaternion per frame."""
        vecs = _f32(vecs)
        N, Vtot, _ = vecs.shape
        nV = Vtot - v0 if nV is None else nV
        out = np.empty((N, nV, 3))
        qq = None if q is None else _f64(q)
        if qq is not None and qq.ndim == 2:
            if qq.shape != (N, 4):
                raise ValueError('per-frame quaternions must have shape (frames, 4)')
            check(self.lib.sr_rotate_vectors_perframe_f32(self.h, _ptr(vecs), N, Vtot, v0, nV, _ptr(qq), _ptr(out)),
                  'sr_rotate_vectors_perframe_f32')
            return out
        check(self.lib.sr_rotate_vectors_f32(self.h, _ptr(vecs), N, Vtot, v0, nV, _ptr(qq), _ptr(out)), 'sr_rotate_vectors_f32')
        return out

    # ---- trajectory front end ----
    def xh_vectors(self, xyz, indexX, indexH, fit_indices=None, ref_xyz=None, want_lab=True, want_quat=False):
        """xyz (nFrames, nAtoms, 3) float32 -> (vec_lab, vec_fit, quat): unit X-H vectors in the lab frame, after the
        per-frame superposition onto ref_xyz over fit_indices (None without a reference), and the rotations."""
        xyz = _f32(xyz)
        if xyz.ndim != 3 or xyz.shape[2] != 3:
            raise ValueError('xyz must be (frames, atoms, 3)')
        nF, nA, _ = xyz.shape
        iX = np.ascontiguousarray(indexX, dtype=np.int32)
        iH = np.ascontiguousarray(indexH, dtype=np.int32)
        if iX.shape != iH.shape or iX.ndim != 1:
            raise ValueError('indexX and indexH must be 1-D and of equal length')
        nV = iX.size
        fit = ref_xyz is not None
        fi = np.ascontiguousarray(fit_indices, dtype=np.int32) if fit else None
        rx = _f32(ref_xyz) if fit else None
        if fit and rx.shape != (nA, 3):
            raise ValueError('ref_xyz must be (atoms, 3)')
        lab = np.empty((nF, nV, 3), dtype=np.float32) if want_lab else None
        fitv = np.empty((nF, nV, 3), dtype=np.float32) if fit else None
        quat = np.empty((nF, 4)) if (fit and want_quat) else None
        check(self.lib.sr_xh_vectors_f32(self.h, _ptr(xyz), nF, nA, _ptr(iX), _ptr(iH), nV, _ptr(fi), fi.size if fit else 0,
                                         _ptr(rx), _ptr(lab), _ptr(fitv), _ptr(quat)), 'sr_xh_vectors_f32')
        return lab, fitv, quat

    # ---- global rotational diffusion (calculate-dq-distribution.py) ----
    def dq_moments(self, q, lags, nchunk=1):
        """q (N, 4) (w x y z), float32 (PLUMED's precision) or float64 (kept as float64: the gmx-rotmat route); lags: frame
        offsets -> (nlags, nchunk, 7) float64: sums of xx yy zz xy xz yz of the vector part of q_i^-1 q_{i+lag} over every
        chunk's samples, and the sample count."""
        q = np.asarray(q)
        f64 = q.dtype == np.float64
        q = _f64(q) if f64 else _f32(q)
        if q.ndim != 2 or q.shape[1] != 4:
            raise ValueError('q must be (N, 4)')
        lg = np.ascontiguousarray(lags, dtype=np.int32)
        out = np.empty((lg.size, int(nchunk), 7))
        fn = self.lib.sr_dq_moments_f64 if f64 else self.lib.sr_dq_moments_f32
        check(fn(self.h, _ptr(q), q.shape[0], _ptr(lg), lg.size, int(nchunk), _ptr(out)), 'sr_dq_moments_f64' if f64 else 'sr_dq_moments_f32')
        return out

    # ---- per-residue CSA refinement of the legacy `--opt new` mode ----
    def legacy_csa_search(self, D, omega, f_DD, gammaB0_sq, time_fact, gamma_ratio, S2, C, tau, nComps, binvecs, weights, expt,
                          csa0, step=1.0, xtol=1e-4, ftol=1e-4, maxiter=1000, maxfun=1000):
        """fmin_powell over the CSA of every residue against its measured (R1, R2, NOE) triple
        (calculate-relaxations-from-Ct.py:210-258, 935-1000): one launch, a workgroup per residue.  D = (Dpar, Dperp); S2 (n),
        C / tau (n, Kmax), nComps (n) already scaled by zeta; binvecs (B, 3), weights (n, B); expt (n, 3, 2) = value and
        uncertainty of R1, R2, NOE; csa0 (n).  Returns csa (n) = Powell's optimum, fopt (n), nfev (n)."""
        Dd = _f64(np.atleast_1d(D))
        om = _f64(np.ravel(omega))
        S2 = _f64(S2)
        n = S2.size
        C, tau = _f64(np.atleast_2d(C)), _f64(np.atleast_2d(tau))
        Kmax = C.shape[1]
        nc = np.ascontiguousarray(nComps, dtype=np.int32)
        bv, w, ex, c0 = _f64(binvecs), _f64(weights), _f64(expt), _f64(csa0)
        B = bv.shape[0]
        if Dd.shape != (2,) or om.shape != (5,):
            raise ValueError('D must be (Dpar, Dperp), omega the 5 angular frequencies')
        if C.shape != (n, Kmax) or tau.shape != (n, Kmax) or nc.shape != (n,) or bv.shape != (B, 3) or w.shape != (n, B) or \
                ex.shape != (n, 3, 2) or c0.shape != (n,):
            raise ValueError('shapes: C / tau (n, Kmax), nComps (n), binvecs (B, 3), weights (n, B), expt (n, 3, 2), csa0 (n)')
        csa, fopt = np.empty(n), np.empty(n)
        nfev = np.empty(n, dtype=np.int32)
        check(self.lib.sr_legacy_csa_search_f64(self.h, _ptr(Dd), _ptr(om), float(f_DD), float(gammaB0_sq), float(time_fact),
                                                float(gamma_ratio), n, Kmax, _ptr(S2), _ptr(C), _ptr(tau), _ptr(nc), B, _ptr(bv),
                                                _ptr(w), _ptr(ex), _ptr(c0), float(step), float(xtol), float(ftol), int(maxiter),
                                                int(maxfun), _ptr(csa), _ptr(fopt), _ptr(nfev)), 'sr_legacy_csa_search_f64')
        return csa, fopt, nfev

    # ---- residue-specific CSA search (new class API) ----
    def rscsa_search(self, stats, column, csa_prefactor, noe_factor, f_DD, target, dtarget, cover, has_err, csa0, step,
                     xtol=1e-4, ftol=1e-4):
        """One-variable Powell search per residue over the closed forms of the 12 statistics (spectral_densities.py:1371-1382,
        1430-1447).  stats (E, n, 12); target/dtarget/cover (E, n).  Returns csa (n), values (E, n), errors (E, n), fopt (n),
        nfev (n)."""
        stats = _f64(stats)
        E, n = stats.shape[0], stats.shape[1]
        if stats.shape != (E, n, 12):
            raise ValueError('stats must be (E, n, 12)')
        col = np.ascontiguousarray(column, dtype=np.int32)
        pref, cn, fdd = _f64(csa_prefactor), _f64(noe_factor), _f64(f_DD)
        y, dy = _f64(target), _f64(dtarget)
        cov = np.ascontiguousarray(cover, dtype=np.uint8)
        c0 = _f64(csa0)
        if col.shape != (E,) or pref.shape != (E,) or cn.shape != (E,) or fdd.shape != (E,):
            raise ValueError('per-experiment arrays must have E entries')
        if y.shape != (E, n) or dy.shape != (E, n) or cov.shape != (E, n) or c0.shape != (n,):
            raise ValueError('target, dtarget and cover must be (E, n), csa0 (n)')
        csa, fopt = np.empty(n), np.empty(n)
        vals, errs = np.empty((E, n)), np.empty((E, n))
        nfev = np.empty(n, dtype=np.int32)
        check(self.lib.sr_rscsa_search_f64(self.h, E, n, _ptr(stats), _ptr(col), _ptr(pref), _ptr(cn), _ptr(fdd), _ptr(y), _ptr(dy),
                                           _ptr(cov), int(bool(has_err)), _ptr(c0), float(step), float(xtol), float(ftol),
                                           _ptr(csa), _ptr(vals), _ptr(errs), _ptr(fopt), _ptr(nfev)), 'sr_rscsa_search_f64')
        return csa, vals, errs, fopt, nfev

    # ---- kernel 3b ----
    def expfit_resjac(self, t, y, sigma, params, want_jac=True):
        t = _f64(np.atleast_2d(t))
        y = _f64(np.atleast_2d(y))
        nRes, L = y.shape
        if t.shape[0] == 1 and nRes > 1:
            t = _f64(np.broadcast_to(t, (nRes, L)))
        s = None if sigma is None else _f64(np.atleast_2d(sigma))
        p = _f64(np.atleast_2d(params))
        P = p.shape[1]
        resid = np.empty((nRes, L))
        jac = np.empty((nRes, L, P)) if want_jac else None
        check(self.lib.sr_expfit_resjac_f64(self.h, _ptr(t), _ptr(y), _ptr(s), _ptr(p), nRes, L, P, _ptr(resid), _ptr(jac)),
              'sr_expfit_resjac_f64')
        return resid, jac

    def expfit_probe(self, t, y, sigma, x, tau_max, jac_mode=0):
        """One evaluation of the fit kernels at x (nRes, P) (sr_expfit_probe_f64): the solver's own model / Jacobian code under the
        current fit_waves / fit_lds / fit_geo.  Returns a dict: geo (nRes), cost (nRes), f (nRes, L), JtJ (nRes, P, P), Jtf (nRes, P),
        dx (nRes, P)."""
        y = _f64(np.atleast_2d(y))
        nRes, L = y.shape
        t = _f64(np.broadcast_to(np.atleast_2d(t), (nRes, L)))
        s = None if sigma is None else _f64(np.broadcast_to(np.atleast_2d(sigma), (nRes, L)))
        x = _f64(np.atleast_2d(x))
        P = x.shape[1]
        out = dict(geo=np.empty(nRes, dtype=np.int32), cost=np.empty(nRes), f=np.empty((nRes, L)), JtJ=np.empty((nRes, P, P)),
                   Jtf=np.empty((nRes, P)), dx=np.empty((nRes, P)))
        check(self.lib.sr_expfit_probe_f64(self.h, _ptr(t), _ptr(y), _ptr(s), _ptr(x), nRes, L, P, float(tau_max), int(jac_mode),
                                           _ptr(out['geo']), _ptr(out['cost']), _ptr(out['f']), _ptr(out['JtJ']), _ptr(out['Jtf']),
                                           _ptr(out['dx'])), 'sr_expfit_probe_f64')
        return out

    def expfit_step_probe(self, x, JtJ, Jtf, Delta, alpha, m, tau_max, mode='step'):
        """One trust-region step of the fit kernels per case (sr_expfit_step_probe_f64): x (n, P), JtJ (n, P, P), Jtf (n, P), Delta,
        alpha, m (n).  mode 'step' returns a dict: v, dv, d, g_h, p_h, step, step_h, xn (n, P), B (n, P, P), g_norm, theta, alpha,
        predicted, step_h_norm, step_norm (n), full_rank, branch, pivot_failures, iterations (n, int32).  mode 'init': x (after
        strictly_feasible(., 1e-10)), v, dv (n, P) and Delta (n)."""
        x = _f64(np.atleast_2d(x))
        n, P = x.shape
        A = _f64(np.asarray(JtJ).reshape(n, P, P))
        g = _f64(np.asarray(Jtf).reshape(n, P))
        De = _f64(np.broadcast_to(np.asarray(Delta, dtype=np.float64), (n,)))
        al = _f64(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (n,)))
        mm = np.ascontiguousarray(np.broadcast_to(np.asarray(m), (n,)), dtype=np.int32)
        vec, B, sca = np.empty((n, 8, P)), np.empty((n, P, P)), np.empty((n, 8))
        flags = np.empty((n, 4), dtype=np.int32)
        check(self.lib.sr_expfit_step_probe_f64(self.h, _ptr(x), _ptr(A), _ptr(g), _ptr(De), _ptr(al), _ptr(mm), n, P, float(tau_max),
                                                {'step': 0, 'init': 1}[mode], _ptr(vec), _ptr(B), _ptr(sca), _ptr(flags)),
              'sr_expfit_step_probe_f64')
        if mode == 'init':
            return dict(x=vec[:, 7].copy(), v=vec[:, 0].copy(), dv=vec[:, 1].copy(), Delta=sca[:, 6].copy())
        out = {k: vec[:, i].copy() for i, k in enumerate(('v', 'dv', 'd', 'g_h', 'p_h', 'step', 'step_h', 'xn'))}
        out.update({k: sca[:, i].copy() for i, k in enumerate(('g_norm', 'theta', 'alpha', 'predicted', 'step_h_norm', 'step_norm'))})
        out.update({k: flags[:, i].copy() for i, k in enumerate(('full_rank', 'branch', 'pivot_failures', 'iterations'))})
        out['B'] = B
        return out

    def expfit(self, t, y, sigma, p0, tau_max, max_nfev=0, analytic_jac=False):
        """Batched bounded fit (scipy curve_fit/TRF semantics).  Returns popt, pcov, chisq, status, nfev."""
        y = _f64(np.atleast_2d(y))
        nRes, L = y.shape
        t = _f64(np.broadcast_to(np.atleast_2d(t), (nRes, L)))
        s = None if sigma is None else _f64(np.broadcast_to(np.atleast_2d(sigma), (nRes, L)))
        p0 = _f64(np.atleast_2d(p0))
        P = p0.shape[1]
        popt = np.empty((nRes, P))
        pcov = np.empty((nRes, P, P))
        chisq = np.empty(nRes)
        status = np.empty(nRes, dtype=np.int32)
        nfev = np.empty(nRes, dtype=np.int32)
        mi = int(max_nfev) if max_nfev else 100 * P
        if analytic_jac:
            mi = -mi
        check(self.lib.sr_expfit_lm_f64(self.h, _ptr(t), _ptr(y), _ptr(s), nRes, L, P, _ptr(p0), float(tau_max), mi,
                                        _ptr(popt), _ptr(pcov), _ptr(chisq), _ptr(status), _ptr(nfev)), 'sr_expfit_lm_f64')
        return popt, pcov, chisq, status, nfev

    def expfit_dev(self, t_ptr, y_ptr, sigma_ptr, nRes, L, P, p0_ptr, tau_max, max_nfev, popt_ptr, pcov_ptr, chisq_ptr,
                   status_ptr, nfev_ptr, skip_ptr=None, work_ptr=None):
        check(self.lib.sr_expfit_lm_f64_dev(self.h, t_ptr, y_ptr, sigma_ptr, nRes, L, P, p0_ptr, float(tau_max),
                                            int(max_nfev), skip_ptr, work_ptr, popt_ptr, pcov_ptr, chisq_ptr, status_ptr, nfev_ptr),
              'sr_expfit_lm_f64_dev')

    def order_search(self, t, y, sigma, orders, tau_guess, tau_max, chi_threshold=0.5):
        """optimised_curve_fitting for (n, L) host arrays in one launch (sr_expfit_order_search_f64).  tau_guess:
        (1 or n, sum(orders)//2... one block of order//2 guesses per order).  Returns a dict of host arrays."""
        t, y = _f64(t), _f64(y)
        n, L = y.shape
        sigma = None if sigma is None else _f64(sigma)
        orders = np.ascontiguousarray(orders, dtype=np.int32)
        nO, Pmax = orders.size, int(orders.max())
        Kmax = Pmax // 2
        tg = _f64(np.atleast_2d(tau_guess))
        out = dict(popt=np.empty((nO, n, Pmax)), dP=np.empty((nO, n, Pmax)), chisq=np.empty((nO, n)),
                   status=np.empty((nO, n), dtype=np.int32), nfev=np.empty((nO, n), dtype=np.int32),
                   best=np.empty(n, dtype=np.int32), S2=np.empty(n), C=np.empty((n, Kmax)), tau=np.empty((n, Kmax)),
                   chi=np.empty(n), K=np.empty(n, dtype=np.int32))
        check(self.lib.sr_expfit_order_search_f64(self.h, _ptr(t), _ptr(y), None if sigma is None else _ptr(sigma), n, L,
                                                  _ptr(orders), nO, _ptr(tg), tg.shape[0], float(tau_max), float(chi_threshold),
                                                  _ptr(out['popt']), _ptr(out['dP']), _ptr(out['chisq']), _ptr(out['status']),
                                                  _ptr(out['nfev']), _ptr(out['best']), _ptr(out['S2']), _ptr(out['C']),
                                                  _ptr(out['tau']), _ptr(out['chi']), _ptr(out['K'])),
              'sr_expfit_order_search_f64')
        out['orders'] = orders
        return out

    def order_search_dev(self, t_ptr, y_ptr, sigma_ptr, nRes, L, orders, tau_guess_ptr, tau_rows, tau_max, chi_threshold,
                         popt_ptr, dP_ptr, chisq_ptr, status_ptr, nfev_ptr, best_ptr, S2_ptr, C_ptr, tau_ptr, chi_ptr, K_ptr,
                         work_ptr=None):
        orders = np.ascontiguousarray(orders, dtype=np.int32)
        check(self.lib.sr_expfit_order_search_f64_dev(self.h, t_ptr, y_ptr, sigma_ptr, nRes, L, _ptr(orders), orders.size,
                                                      tau_guess_ptr, tau_rows, float(tau_max), float(chi_threshold), work_ptr,
                                                      popt_ptr, dP_ptr, chisq_ptr, status_ptr, nfev_ptr, best_ptr, S2_ptr, C_ptr,
                                                      tau_ptr, chi_ptr, K_ptr), 'sr_expfit_order_search_f64_dev')

    # ---- signals (a stream waits for a value a kernel writes) ----
    def signal_alloc(self):
        p = self.lib.sr_signal_alloc(self.h)
        if not p:
            raise SpinRelaxHipError('sr_signal_alloc failed: %s' % _lib.last_error())
        return p

    def signal_free(self, sig):
        check(self.lib.sr_signal_free(self.h, sig), 'sr_signal_free')

    def stream_wait_signal(self, sig, value):
        check(self.lib.sr_stream_wait_signal(self.h, sig, int(value)), 'sr_stream_wait_signal')

    def stream_write_signal(self, sig, value):
        check(self.lib.sr_stream_write_signal(self.h, sig, int(value)), 'sr_stream_write_signal')

    def order_search_batched_dev(self, t_ptr, t_rows, y_ptr, sigma_ptr, nRes, L, orders, tau_guess_ptr, tau_rows, tau_max, chi_threshold,
                                 popt_ptr, dP_ptr, chisq_ptr, status_ptr, nfev_ptr, best_ptr, S2_ptr, C_ptr, tau_ptr, chi_ptr, K_ptr,
                                 work_ptr=None, dispatch_order_ptr=None, tail_signal=None, tail_value=0):
        """the model-order search of several batches' residues in one launch (sr_expfit_order_search_batched_f64_dev):
        t_rows = 1 shares one time axis, dispatch_order (device int32, nRes) permutes the order in which residues start"""
        orders = np.ascontiguousarray(orders, dtype=np.int32)
        check(self.lib.sr_expfit_order_search_batched_f64_dev(self.h, t_ptr, t_rows, y_ptr, sigma_ptr, nRes, L, _ptr(orders), orders.size,
                                                              tau_guess_ptr, tau_rows, float(tau_max), float(chi_threshold),
                                                              dispatch_order_ptr, tail_signal, int(tail_value), work_ptr, popt_ptr, dP_ptr,
                                                              chisq_ptr, status_ptr,
                                                              nfev_ptr, best_ptr, S2_ptr, C_ptr, tau_ptr, chi_ptr, K_ptr),
              'sr_expfit_order_search_batched_f64_dev')

    def order_search_sums_dev(self, t_ptr, t_rows, sums_ptr, R, F, CtT_ptr, dCtT_ptr, nRes, L, orders, tau_guess_ptr, tau_rows, tau_max,
                              chi_threshold, popt_ptr, dP_ptr, chisq_ptr, status_ptr, nfev_ptr, best_ptr, S2_ptr, C_ptr, tau_ptr, chi_ptr,
                              K_ptr, work_ptr=None, dispatch_order_ptr=None, tail_signal=None, tail_value=0, refusal_ok=False):
        """order_search_batched_dev on kernel 1's raw sums (nRes, R, psum_stride(F)): the launch computes the chunk statistics of
        every residue itself and writes C(t) / dC(t) to CtT_ptr / dCtT_ptr (nRes, L) (sr_expfit_order_search_sums_f64_dev).
        refusal_ok: a refusal of the arguments (-2, -3: nothing has been queued) is returned instead of raised, so that the caller
        can take the two-launch path; returns 0 otherwise"""
        orders = np.ascontiguousarray(orders, dtype=np.int32)
        rc = self.lib.sr_expfit_order_search_sums_f64_dev(self.h, t_ptr, t_rows, sums_ptr, int(R), int(F), CtT_ptr, dCtT_ptr, nRes, L,
                                                          _ptr(orders), orders.size, tau_guess_ptr, tau_rows, float(tau_max),
                                                          float(chi_threshold), dispatch_order_ptr, tail_signal, int(tail_value),
                                                          work_ptr, popt_ptr, dP_ptr, chisq_ptr, status_ptr, nfev_ptr, best_ptr, S2_ptr,
                                                          C_ptr, tau_ptr, chi_ptr, K_ptr)
        if refusal_ok and rc in (-2, -3):
            return rc
        check(rc, 'sr_expfit_order_search_sums_f64_dev')
        return 0

    def relax_dev(self, model, D, E, omega_ptr, fDD_ptr, fCSA_ptr, tf_ptr, gr_ptr, nRes, Kmax, zeta, S2_ptr, C_ptr, tau_ptr,
                  K_ptr, B, binvecs_ptr, weights_ptr, noe_mode, out_ptr, Jout_ptr=None, stats_ptr=None):
        """Context.relax on device pointers (sr_jomega_relax_f64_dev); model and D as there, model 3 = [Dx, Dy, Dz]"""
        Dh = _f64(np.atleast_1d(D))
        if model == 3 and Dh.size != 3:
            raise ValueError('ellipsoid model needs D = [Dx, Dy, Dz]')
        check(self.lib.sr_jomega_relax_f64_dev(self.h, model, _ptr(Dh), E, omega_ptr, fDD_ptr, fCSA_ptr, tf_ptr, gr_ptr, nRes,
                                               Kmax, float(zeta), S2_ptr, C_ptr, tau_ptr, K_ptr, B, binvecs_ptr, weights_ptr,
                                               noe_mode, out_ptr, Jout_ptr, stats_ptr), 'sr_jomega_relax_f64_dev')

    def transpose_dev(self, in_ptr, rows, cols, out_ptr):
        check(self.lib.sr_transpose_f64_dev(self.h, in_ptr, rows, cols, out_ptr), 'sr_transpose_f64_dev')

    def transpose_batched_dev(self, in_ptr, g, rows, cols, out_ptr):
        """g contiguous (rows, cols) matrices, each to (cols, rows), in one launch (sr_transpose_batched_f64_dev)"""
        check(self.lib.sr_transpose_batched_f64_dev(self.h, in_ptr, int(g), int(rows), int(cols), out_ptr), 'sr_transpose_batched_f64_dev')

    # ---- kernel 3a ----
    def jomega(self, x, y):
        x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
        xs = _f64(x)
        ys = _f64(y)
        out = np.empty(xs.shape)
        check(self.lib.sr_jomega_f64(self.h, _ptr(xs), _ptr(ys), _ptr(out), xs.size), 'sr_jomega_f64')
        return out

    def relax(self, model, D, omega, f_DD, f_CSA, time_fact, gamma_ratio, S2, C, tau, nComps,
              binvecs=None, weights=None, resvecs=None, noe_mode=0, want_J=False, weights_dev_ptr=None, want_stats=False):
        """model 0 direct / 1 sphere (D=[Diso]) / 2 symmetric top (D=[Dpar, Dperp]) / 3 rhombic ellipsoid (D=[Dx, Dy, Dz],
        the principal values along the x, y, z axes of the frame the vectors are in).
        Symmetric top and ellipsoid: either `binvecs` (B,3) shared by all residues with optional `weights` (nRes,B), or
        `resvecs` (nRes,3), one vector per residue.  Returns out (E, nRes, 4, 2) = [R1,R2,NOE,rho] x
        [mean, sigma] and J (E, nRes, 5, 2) or None."""
        omega = _f64(np.atleast_2d(omega))
        E = omega.shape[0]
        S2 = _f64(S2)
        nRes = S2.size
        C = _f64(np.atleast_2d(C))
        tau = _f64(np.atleast_2d(tau))
        Kmax = C.shape[1]
        f_DD = _f64(np.broadcast_to(f_DD, (E,)))
        f_CSA = _f64(np.broadcast_to(f_CSA, (E, nRes)))
        time_fact = _f64(np.broadcast_to(time_fact, (E,)))
        gamma_ratio = _f64(np.broadcast_to(gamma_ratio, (E,)))
        nc = np.ascontiguousarray(nComps, dtype=np.int32)
        Dd = None if D is None else _f64(np.atleast_1d(D))
        B = 0
        bv = None
        w = None
        if model == 3 and (Dd is None or Dd.size != 3):
            raise ValueError('ellipsoid model needs D = [Dx, Dy, Dz]')
        if model in (2, 3):
            if binvecs is not None:
                bv = _f64(binvecs)
                B = bv.shape[0]
                if weights is not None:
                    w = _f64(weights)
                    if w.shape != (nRes, B):
                        raise ValueError('weights must be (nRes, B)')
            elif resvecs is not None:
                bv = _f64(resvecs)
                if bv.shape != (nRes, 3):
                    raise ValueError('resvecs must be (nRes, 3)')
            else:
                raise ValueError('symmetric-top and ellipsoid models need binvecs or resvecs')
        out = np.empty((E, nRes, 4, 2))
        J = np.empty((E, nRes, 5, 2)) if want_J else None
        stats = np.empty((E, nRes, 12)) if want_stats else None
        check(self.lib.sr_jomega_relax_f64(self.h, int(model), _ptr(Dd), E, _ptr(omega), _ptr(f_DD), _ptr(f_CSA),
                                           _ptr(time_fact), _ptr(gamma_ratio), nRes, Kmax, _ptr(S2), _ptr(C), _ptr(tau),
                                           _ptr(nc), B, _ptr(bv), weights_dev_ptr if weights_dev_ptr else _ptr(w),
                                           1 if weights_dev_ptr else 0, int(noe_mode), _ptr(out), _ptr(J), _ptr(stats)),
              'sr_jomega_relax_f64')
        if want_stats:
            return out, J, stats
        return out, J


_default = {}


def _close_default_contexts():
    for c in list(_default.values()):
        try:
            c.close()
        except Exception:
            pass
    _default.clear()


import atexit as _atexit      # noqa: E402
_atexit.register(_close_default_contexts)      # teardown while the HIP runtime is still alive, not from __del__ at exit


def default_context(device=None):
    """Process-wide context per device (created on first use).  Without an explicit device: SPINRELAX_DEVICE, else the
    LOCAL_RANK torchrun sets (one rank per GPU), else 0."""
    if device is None:
        import os
        device = int(os.environ.get('SPINRELAX_DEVICE', os.environ.get('LOCAL_RANK', '0')))
    if device not in _default or _default[device].h is None:
        _default[device] = Context(device)
    return _default[device]


class ResidentVectors:
    """One rank's columns [v0, v0 + nV) of a (frames, vectors, 3) float32 array on the device: appended chunk by chunk
    (strided host copies of just those columns, or straight from coordinates through the GPU front end), packed once,
    then read by C(t) and by the rotation + histogram pass.  sr_vectors_* of include/spinrelax_hip.h."""

    def __init__(self, ctx, nV, capacity=0):
        self.ctx = ctx
        self.nV = int(nV)
        self.h = ctx.lib.sr_vectors_create(ctx.h, self.nV, int(capacity))
        if not self.h:
            raise SpinRelaxHipError('sr_vectors_create failed: %s' % _lib.last_error())

    def close(self):
        if getattr(self, 'h', None) and getattr(self.ctx, 'h', None):
            self.ctx.lib.sr_vectors_destroy(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def frames(self):
        return int(self.ctx.lib.sr_vectors_frames(self.h))

    def append(self, vecs, v0=0):
        """n more frames from a host array (n, Vtot, 3); only columns [v0, v0 + nV) are copied to the device"""
        vecs = _f32(vecs)
        if vecs.ndim != 3 or vecs.shape[2] != 3:
            raise ValueError('vecs must be (frames, vectors, 3)')
        check(self.ctx.lib.sr_vectors_append_f32(self.ctx.h, self.h, _ptr(vecs), vecs.shape[0], vecs.shape[1], int(v0)),
              'sr_vectors_append_f32')
        return self

    def truncate(self, n_frames):
        check(self.ctx.lib.sr_vectors_truncate(self.ctx.h, self.h, int(n_frames)), 'sr_vectors_truncate')

    def append_pinned(self, host_addr, n, Vtot, v0=0):
        """n more frames from PAGE-LOCKED host memory at `host_addr` ((n, Vtot, 3) float32): one asynchronous copy on the
        context's current stream, no staging pass; the memory must stay unchanged until the stream has passed this point"""
        check(self.ctx.lib.sr_vectors_append_f32(self.ctx.h, self.h, ctypes.c_void_p(int(host_addr)), int(n), int(Vtot), int(v0)),
              'sr_vectors_append_f32')
        return self

    def device_ptr(self):
        """device address of the (frames, nV, 3) float32 array; work queued on the context's stream behind this call sees
        every appended frame"""
        p = self.ctx.lib.sr_vectors_frame_major_dev(self.ctx.h, self.h)
        if not p:
            raise SpinRelaxHipError('sr_vectors_frame_major_dev failed: %s' % _lib.last_error())
        return int(p)

    def download(self, f0=0, n=None):
        n = self.frames - f0 if n is None else n
        out = np.empty((n, self.nV, 3), dtype=np.float32)
        check(self.ctx.lib.sr_vectors_download_f32(self.ctx.h, self.h, int(f0), int(n), _ptr(out)), 'sr_vectors_download_f32')
        return out

    def ct(self, R, F, chunk_start=None, mode=0):
        """calculate_Ct_Palmer (calculate-Ct-from-traj.py:200-238) of the resident vectors: Ct, dCt (F//2, nV) float64"""
        L = F // 2
        Ct = np.empty((L, self.nV))
        dCt = np.empty((L, self.nV))
        cs = _chunk_starts(chunk_start, R)
        check(self.ctx.lib.sr_vectors_ct_f32(self.ctx.h, self.h, int(R), int(F), _ptr(cs), int(mode), _ptr(Ct), _ptr(dCt)),
              'sr_vectors_ct_f32')
        return Ct, dCt

    def ct_cross(self, R, F, pairs, chunk_start=None, sym=1, mode=0, want_dP0=False):
        """time-lagged P2 cross-correlation of the pairs (nP, 2) of resident vectors (sr_vectors_ct_cross_f32): P0 (nP) the equal-time
        <P2(u_i . u_j)>, Ct and dCt (F//2, nP) = <P2(u_i(t) . u_j(t + k))>, k = 1 .. F//2, mean and error over the R chunks like ct();
        sym = 1: the mean of C_ij and C_ji.  want_dP0: (P0, dP0, Ct, dCt), dP0 the error of P0 over the chunks (sr_vectors_ct_cross_err_f32)"""
        return self._ct_cross('sr_vectors_ct_cross', R, F, pairs, chunk_start, sym, mode, want_dP0)

    def ct_cross_long(self, R, F, pairs, chunk_start=None, sym=1, mode=0, want_dP0=False):
        """ct_cross for chunks of 5462 .. Context.ct_cross_long_max_frames() frames, by blocked transforms (sr_vectors_ct_cross_long_f32,
        sr_vectors_ct_cross_long_err_f32): the same arguments and results"""
        return self._ct_cross('sr_vectors_ct_cross_long', R, F, pairs, chunk_start, sym, mode, want_dP0)

    def _ct_cross(self, stem, R, F, pairs, chunk_start, sym, mode, want_dP0):
        pi, pj = pair_columns(pairs)
        L = F // 2
        P0 = np.empty(pi.size)
        Ct = np.empty((L, pi.size))
        dCt = np.empty((L, pi.size))
        cs = _chunk_starts(chunk_start, R)
        out = (P0, np.empty(pi.size), Ct, dCt) if want_dP0 else (P0, Ct, dCt)
        name = stem + ('_err_f32' if want_dP0 else '_f32')
        check(getattr(self.ctx.lib, name)(self.ctx.h, self.h, int(R), int(F), _ptr(cs), _ptr(pi), _ptr(pj), pi.size, int(sym), int(mode),
                                          *[_ptr(a) for a in out]), name)
        return out

    def ct_dipolar(self, R, F, dist=None, chunk_start=None, mode=0):
        """distance-weighted dipolar correlation function of the resident vectors (sr_vectors_ct_dipolar_f32):
        C_dd(k) = <P2(u(t) . u(t+k)) r(t)^-3 r(t+k)^-3> / <r^-6>, k = 1 .. F//2, mean and error over the R chunks like ct().  dist
        (frames held, nV): the distances, the vectors then give the direction only; None: the length of a vector is its distance.
        Returns Ct, dCt (F//2, nV) and per vector reff6 = <r^-6>^(-1/6), reff3 = <r^-3>^(-1/3), S2rad = <r^-3>^2 / <r^-6>."""
        return self._ct_dipolar('sr_vectors_ct_dipolar_f32', R, F, dist, chunk_start, mode)

    def ct_dipolar_long(self, R, F, dist=None, chunk_start=None, mode=0):
        """ct_dipolar for chunks of 5462 .. Context.ct_dipolar_long_max_frames() frames, by blocked transforms
        (sr_vectors_ct_dipolar_long_f32): the same arguments and results"""
        return self._ct_dipolar('sr_vectors_ct_dipolar_long_f32', R, F, dist, chunk_start, mode)

    def _held_dist(self, dist):
        """a distance array as the library takes it: None, or float32 of the shape (frames held, vectors)"""
        if dist is None:
            return None
        d = _f32(dist)
        if d.shape != (self.frames, self.nV):
            raise ValueError('dist must be (frames held, vectors) = (%d, %d), got %s' % (self.frames, self.nV, d.shape))
        return d

    def _ct_dipolar(self, name, R, F, dist, chunk_start, mode):
        L = F // 2
        d = self._held_dist(dist)
        Ct = np.empty((L, self.nV))
        dCt = np.empty((L, self.nV))
        reff6, reff3, S2rad = np.empty(self.nV), np.empty(self.nV), np.empty(self.nV)
        cs = _chunk_starts(chunk_start, R)
        check(getattr(self.ctx.lib, name)(self.ctx.h, self.h, _ptr(d), int(R), int(F), _ptr(cs), int(mode), _ptr(Ct), _ptr(dCt), _ptr(reff6),
                                          _ptr(reff3), _ptr(S2rad)), name)
        return Ct, dCt, reff6, reff3, S2rad

    def ct_modes(self, R, F, frame=None, chunk_start=None, mode=0):
        """the six mode sums of the resident vectors in the frame R(frame) (sr_vectors_ct_modes_f32): H, dH (F//2 + 1, nV, 6) for the
        lags 0 .. F//2, mean and error over the R chunks like ct(), and smean (nV, 5), the means of the five signals.  frame: a unit
        quaternion (w, x, y, z), --vecRot's convention, or None.  Chunks of up to Context.ct_modes_max_frames() frames."""
        fq = Context._frame(frame)
        L1 = F // 2 + 1
        H = np.empty((L1, self.nV, 6))
        dH = np.empty((L1, self.nV, 6))
        smean = np.empty((self.nV, 5))
        cs = _chunk_starts(chunk_start, R)
        check(self.ctx.lib.sr_vectors_ct_modes_f32(self.ctx.h, self.h, _ptr(fq), int(R), int(F), _ptr(cs), int(mode), _ptr(H), _ptr(dH),
                                                   _ptr(smean)), 'sr_vectors_ct_modes_f32')
        return H, dH, smean

    def ct_dipolar_cross(self, R, F, pairs, dist=None, chunk_start=None, sym=1, mode=0):
        """distance-weighted P2 cross-correlation of the pairs (nP, 2) of resident vectors (sr_vectors_ct_dipolar_cross_f32):
        C_ij(k) = <P2(u_i(t) . u_j(t+k)) r_i(t)^-3 r_j(t+k)^-3> / sqrt(<r_i^-6> <r_j^-6>), k = 1 .. F//2, mean and error over the R chunks
        like ct(); sym = 1: the mean of C_ij and C_ji.  dist as in ct_dipolar.  Returns (P0, dP0, Ct, dCt, reff6): P0, dP0 (nP) the
        equal-time value and its error, Ct, dCt (F//2, nP), reff6 (nP, 2) = <r^-6>^(-1/6) of the two vectors of each pair."""
        return self._ct_dipolar_cross('sr_vectors_ct_dipolar_cross_f32', R, F, pairs, dist, chunk_start, sym, mode)

    def ct_dipolar_cross_long(self, R, F, pairs, dist=None, chunk_start=None, sym=1, mode=0):
        """ct_dipolar_cross for chunks of 4097 .. Context.ct_dipolar_cross_long_max_frames() frames, by blocked transforms
        (sr_vectors_ct_dipolar_cross_long_f32): the same arguments and results"""
        return self._ct_dipolar_cross('sr_vectors_ct_dipolar_cross_long_f32', R, F, pairs, dist, chunk_start, sym, mode)

    def _ct_dipolar_cross(self, name, R, F, pairs, dist, chunk_start, sym, mode):
        pi, pj = pair_columns(pairs)
        L = F // 2
        d = self._held_dist(dist)
        P0, dP0 = np.empty(pi.size), np.empty(pi.size)
        Ct = np.empty((L, pi.size))
        dCt = np.empty((L, pi.size))
        reff6 = np.empty((pi.size, 2))
        cs = _chunk_starts(chunk_start, R)
        check(getattr(self.ctx.lib, name)(self.ctx.h, self.h, _ptr(d), int(R), int(F), _ptr(cs), _ptr(pi), _ptr(pj), pi.size, int(sym), int(mode),
                                          _ptr(P0), _ptr(dP0), _ptr(Ct), _ptr(dCt), _ptr(reff6)), name)
        return P0, dP0, Ct, dCt, reff6

    def ct_sums(self, R, F, chunk_start=None, mode=0):
        """raw sums S[v, r, d-1] = sum_j (u_j . u_{j+d})^2 of the R chunks held, (nV, R, F//2) float64 (replicate sharding)"""
        sums = np.empty((self.nV, R, F // 2))
        cs = _chunk_starts(chunk_start)
        check(self.ctx.lib.sr_vectors_ct_sums_f32(self.ctx.h, self.h, int(R), int(F), _ptr(cs), int(mode), _ptr(sums)),
              'sr_vectors_ct_sums_f32')
        return sums

    def hist(self, q, edges_phi, edges_cos, block_len=0, N_hist=0, want_outer=True):
        """rotation + Lambert histogram + vector sums + per-block outer-product sums (calculate-Ct-from-traj.py:541-646) of
        the first N_hist frames (0 = all): hist (nV, nphi, ncos), vecsum (nV, 3), outer (nB, nV, 6)"""
        ep = _f64(edges_phi)
        ec = _f64(edges_cos)
        nphi, ncos = ep.size - 1, ec.size - 1
        qq = None if q is None else _f64(q)
        N = N_hist if N_hist and N_hist > 0 else self.frames
        hist = np.empty((self.nV, nphi, ncos))
        vecsum = np.empty((self.nV, 3))
        Fb = block_len if (block_len and 0 < block_len <= N) else N
        outer = np.empty((N // Fb, self.nV, 6)) if want_outer else None
        check(self.ctx.lib.sr_vectors_hist_f32(self.ctx.h, self.h, int(N), _ptr(qq), _ptr(ep), nphi, _ptr(ec), ncos, _ptr(hist),
                                               _ptr(vecsum), _ptr(outer), int(block_len or 0)), 'sr_vectors_hist_f32')
        return hist, vecsum, outer

    def ired(self, win_start, win_len):
        """iRED matrices of the resident vectors: M (W, nV, nV) float64, M[w][i][j] = mean over the frames
        [win_start[w], win_start[w] + win_len[w]) of 1.5 (u_i . u_j)^2 - 0.5 (sr_vectors_ired_f32)"""
        ws, wl = _windows(win_start, win_len)
        M = np.empty((ws.size, self.nV, self.nV))
        check(self.ctx.lib.sr_vectors_ired_f32(self.ctx.h, self.h, _ptr(ws), _ptr(wl), ws.size, _ptr(M)), 'sr_vectors_ired_f32')
        return M

    def ired_mode_ct(self, win_start, win_len, coef, n_lags):
        """iRED mode correlation functions of the resident vectors: coef (W, K, nV) float64, row m of window w the weights e_mi
        of one mode -> Cm (W, K, n_lags) float64,
        Cm[w][m][k] = sum_ij e_mi e_mj < 1.5 (u_i(t) . u_j(t + k))^2 - 0.5 >_t over the window (sr_vectors_ired_mode_ct_f32)"""
        ws, wl = _windows(win_start, win_len)
        coef = _f64(coef)
        if coef.ndim != 3 or coef.shape[0] != ws.size or coef.shape[2] != self.nV:
            raise ValueError('coef must be (windows, modes, vectors) = (%d, K, %d)' % (ws.size, self.nV))
        K, n_lags = coef.shape[1], int(n_lags)
        Cm = np.empty((ws.size, K, max(n_lags, 0)))
        check(self.ctx.lib.sr_vectors_ired_mode_ct_f32(self.ctx.h, self.h, _ptr(ws), _ptr(wl), ws.size, _ptr(coef), K, n_lags, _ptr(Cm)),
              'sr_vectors_ired_mode_ct_f32')
        return Cm


def append_xyz(ctx, lab, fit, xyz, indexX, indexH, fit_indices=None, ref_xyz=None):
    """obtain_XHvecs (+ centring and superposition when fit_indices / ref_xyz are given) of one chunk of coordinates
    (frames, atoms, 3) on the GPU, appended to the ResidentVectors objects `lab` and / or `fit` (either may be None);
    indexX / indexH are THIS rank's slice of the selections.  calculate-Ct-from-traj.py:64-86, 462-470."""
    xyz = _f32(xyz)
    iX = np.ascontiguousarray(indexX, dtype=np.int32)
    iH = np.ascontiguousarray(indexH, dtype=np.int32)
    fi = None if fit_indices is None else np.ascontiguousarray(fit_indices, dtype=np.int32)
    rx = None if ref_xyz is None else _f32(ref_xyz)
    check(ctx.lib.sr_vectors_append_xyz_f32(ctx.h, None if lab is None else lab.h, None if fit is None else fit.h, _ptr(xyz),
                                            xyz.shape[0], xyz.shape[1], _ptr(iX), _ptr(iH), iX.size, _ptr(fi),
                                            0 if fi is None else fi.size, _ptr(rx)), 'sr_vectors_append_xyz_f32')
