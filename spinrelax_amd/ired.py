"""
iRED order parameters (isotropic reorientational eigenmode dynamics): S2 of every bond vector from the equal-time P2
cross-correlation matrix of all of them, with no superposition, no de-tumbling and no fit.

    M_w[i][j] = mean over the frames of window w of  1.5 (u_i(t) . u_j(t))^2 - 0.5
    M_w = sum_m lambda_m |m><m|, lambda descending;   S2_w[i] = 1 - sum_{m > G} lambda_m |m>_i^2,   G = 5 global modes

(Prompers & Brueschweiler, J. Am. Chem. Soc. 124, 4522 (2002); windows for long trajectories: Gu, Li & Brueschweiler,
J. Chem. Theory Comput. 10, 2599 (2014)).  The reference announces the analysis in calculate_S2_by_iRED / calculate_S2_by_wiRED
(calculate-S2.py:158-191) and stops after the window length; this module is built to the publications and keeps the reference's
conventions where it has any: windows tile every file like reformat_vecs_by_tau, the stub's window of 5 tau, and the error
convention of calculate_S2_by_outerProduct.

The dynamics of the modes (mode_ct=True): the trajectory is projected on the eigenvectors of its window,

    C_m(k) = sum_ij |m>_i |m>_j < 1.5 (u_i(t) . u_j(t + k))^2 - 0.5 >_t,   C_m(0) = lambda_m;   tau_m = dt * integral of C_m / C_m(0)
    C_i(k) = sum_m |m>_i^2 C_m(k)                 (the correlation function of vector i: no separability assumption, no de-tumbling)

M and C_m(k), the loops that are quadratic in the number of vectors, are computed on the MI355X (csrc/sr_ired.hip,
csrc/sr_ired_modes.hip) and nowhere else: there is no CPU path for them, without a GPU the calls raise SpinRelaxHipError.  The
eigen-decomposition of the (N, N) matrices is numpy.linalg.eigh on the host.
"""
import numpy as np

from . import hip


def _ctx(ctx):
    return ctx if ctx is not None else hip.default_context()


def ired_windows(frames_per_file, dt, window=None, tau=None):
    """(win_start, win_len), int64: windows of F_w = int(window / dt) frames tile every file from its first frame, a tail that
    does not fill a window is dropped, no window spans two files (the rule of reformat_vecs_by_tau,
    calculate-Ct-from-traj.py:245-275); starts count frames of the concatenated files.  window None: 5 tau when tau is given
    (calculate-S2.py:162), otherwise one window per file, the whole file."""
    frames = [int(n) for n in frames_per_file]
    if window is None and tau is not None:
        window = 5.0 * tau
    starts, lens, off = [], [], 0
    if window is None:
        for n in frames:
            if n > 0:
                starts.append(off)
                lens.append(n)
            off += n
    else:
        Fw = int(window / dt)
        if Fw < 1:
            raise ValueError('ired_windows: a window of %g holds no frame at dt = %g' % (window, dt))
        for n in frames:
            for c in range(n // Fw):
                starts.append(off + c * Fw)
                lens.append(Fw)
            off += n
    return np.array(starts, dtype=np.int64), np.array(lens, dtype=np.int64)


def ired_S2(M, n_global=5):
    """M (W, N, N) (or (N, N)) -> S2_w (W, N), lam_w (W, N): per window the eigenvalues in descending order and
    S2[i] = 1 - sum_{m > n_global} lam_m |m>_i^2, the n_global largest modes being overall tumbling."""
    M = np.asarray(M, dtype=np.float64)
    if M.ndim == 2:
        M = M[np.newaxis]
    if M.ndim != 3 or M.shape[1] != M.shape[2]:
        raise ValueError('ired_S2: M must be (windows, N, N)')
    N = M.shape[1]
    if N <= n_global:
        raise ValueError('ired_S2: %d vectors do not exceed the %d global modes' % (N, n_global))
    lam, vec = np.linalg.eigh(M)                      # ascending; columns are the modes
    lam, vec = lam[:, ::-1], vec[:, :, ::-1]
    S2 = 1.0 - np.einsum('wm,wim->wi', lam[:, n_global:], vec[:, :, n_global:] ** 2)
    return S2, np.ascontiguousarray(lam)


def ired_S2_modes(M, n_global=5):
    """ired_S2 that keeps the eigenvectors: S2_w (W, N), lam_w (W, N), modes_w (W, N, N) with modes_w[w][m] = |m> of window w,
    the modes as ROWS in the order of lam_w (the coefficient matrices of hip.ResidentVectors.ired_mode_ct)."""
    M = np.asarray(M, dtype=np.float64)
    if M.ndim == 2:
        M = M[np.newaxis]
    if M.ndim != 3 or M.shape[1] != M.shape[2]:
        raise ValueError('ired_S2_modes: M must be (windows, N, N)')
    if M.shape[1] <= n_global:
        raise ValueError('ired_S2_modes: %d vectors do not exceed the %d global modes' % (M.shape[1], n_global))
    lam, vec = np.linalg.eigh(M)                      # the call and the reversal of ired_S2: the same bits
    lam, vec = lam[:, ::-1], vec[:, :, ::-1]
    S2 = 1.0 - np.einsum('wm,wim->wi', lam[:, n_global:], vec[:, :, n_global:] ** 2)
    return S2, np.ascontiguousarray(lam), np.ascontiguousarray(np.swapaxes(vec, 1, 2))


def ired_mode_tau(Cm, dt):
    """Cm (..., n_lags) -> tau (...): dt times the trapezoid sum of C_m(k) / C_m(0) from k = 0 to the last lag before the first k
    with C_m(k) <= 0 (to the last lag when there is none); 0 for a mode with C_m(0) <= 0."""
    Cm = np.asarray(Cm, dtype=np.float64)
    flat = Cm.reshape(-1, Cm.shape[-1])
    tau = np.zeros(flat.shape[0])
    for m, c in enumerate(flat):
        if c[0] <= 0.0:
            continue
        neg = np.nonzero(c <= 0.0)[0]
        c = c[:neg[0]] if neg.size else c
        tau[m] = dt * (c.sum() - 0.5 * (c[0] + c[-1])) / c[0]
    return tau.reshape(Cm.shape[:-1])


def ired_vector_ct(vec, Cm):
    """vec (..., N, K) with vec[i][m] = |m>_i (modes as COLUMNS, what numpy.linalg.eigh returns), Cm (..., K, n_lags) ->
    C_i(k) = sum_m vec[i][m]^2 C_m(k), (..., N, n_lags), over all modes."""
    vec, Cm = np.asarray(vec, dtype=np.float64), np.asarray(Cm, dtype=np.float64)
    if vec.shape[-1] != Cm.shape[-2]:
        raise ValueError('ired_vector_ct: vec has %d modes, Cm %d' % (vec.shape[-1], Cm.shape[-2]))
    return np.einsum('...im,...mk->...ik', vec * vec, Cm)


IRED_MAX_TRANSFORM = 8192      # the longest in-LDS transform of k_ired_mode_ct: F_w + n_lags - 1 may not exceed it


def ired_reduce(S2_w):
    """S2_w (W, N) -> S2 = mean over the windows, dS2 = std(ddof = 0) / (sqrt(W) - 1) (the error convention of
    calculate_S2_by_outerProduct, calculate-Ct-from-traj.py:138-142); dS2 = 0 for a single window."""
    S2_w = np.atleast_2d(np.asarray(S2_w, dtype=np.float64))
    W = S2_w.shape[0]
    S2 = S2_w.mean(axis=0)
    if W == 1:
        return S2, np.zeros_like(S2)
    return S2, S2_w.std(axis=0) / (np.sqrt(W) - 1.0)


def _analyse(M, win_start, win_len, n_global):
    S2_w, lam_w = ired_S2(M, n_global)
    S2, dS2 = ired_reduce(S2_w)
    return dict(S2=S2, dS2=dS2, eig=lam_w.mean(axis=0), S2_w=S2_w, lam_w=lam_w, M=M, win_start=win_start, win_len=win_len)


def calculate_iRED_resident(rv, frames_per_file, dt, window=None, tau=None, n_global=5, mode_ct=False, n_lags=None):
    """iRED of resident vectors (hip.ResidentVectors) that hold the files one after the other, frames_per_file frames of each.
    Returns a dict: S2, dS2 (N), eig (N) = the eigenvalues averaged over the windows per rank, S2_w, lam_w (W, N), M (W, N, N),
    win_start, win_len.
    mode_ct=True adds the dynamics: modes_w (W, N, N) the eigenvectors as rows, Cm_w (W, N, n_lags) the correlation function of
    every mode, Cm (N, n_lags) its mean over the windows per rank (like eig), tau (N) = ired_mode_tau(Cm, dt), and Ct_vec, dCt_vec
    (n_lags, N): the mean over the windows of C_i(k) = sum_m |m>_i^2 C_m(k) and its std / (sqrt(W) - 1).  n_lags defaults to
    F_w // 2 + 1 (lags 0 .. F_w // 2); all windows must have one length F_w, and F_w + n_lags - 1 may not exceed 8192."""
    if rv.nV <= n_global:
        raise ValueError('iRED: %d vectors do not exceed the %d global modes' % (rv.nV, n_global))
    win_start, win_len = ired_windows(frames_per_file, dt, window=window, tau=tau)
    if win_start.size < 1:
        raise ValueError('iRED: no file holds a whole window')
    if not mode_ct:
        return _analyse(rv.ired(win_start, win_len), win_start, win_len, n_global)
    Fw = int(win_len[0])
    if np.any(win_len != Fw):
        raise ValueError('iRED mode correlation functions need windows of one length (got %d to %d frames): give a window '
                         '(--iRED_window) or a memory time' % (win_len.min(), win_len.max()))
    n_lags = Fw // 2 + 1 if n_lags is None else int(n_lags)
    if n_lags < 1 or n_lags > Fw:
        raise ValueError('iRED: n_lags = %d is outside 1 .. %d, the frames of a window' % (n_lags, Fw))
    if Fw + n_lags - 1 > IRED_MAX_TRANSFORM:
        raise ValueError('iRED mode correlation functions: windows of %d frames with %d lags need a transform of %d points, the '
                         'longest is %d; shorten the window (--iRED_window), at most 5461 frames with the default lags'
                         % (Fw, n_lags, Fw + n_lags - 1, IRED_MAX_TRANSFORM))
    M = rv.ired(win_start, win_len)
    S2_w, lam_w, modes_w = ired_S2_modes(M, n_global)
    S2, dS2 = ired_reduce(S2_w)
    Cm_w = rv.ired_mode_ct(win_start, win_len, modes_w, n_lags)
    Cm = Cm_w.mean(axis=0)
    Ct_w = ired_vector_ct(np.swapaxes(modes_w, 1, 2), Cm_w)            # (W, N, n_lags)
    Ct_vec, dCt_vec = ired_reduce(Ct_w.reshape(Ct_w.shape[0], -1))
    shape = Ct_w.shape[1:]
    return dict(S2=S2, dS2=dS2, eig=lam_w.mean(axis=0), S2_w=S2_w, lam_w=lam_w, M=M, win_start=win_start, win_len=win_len,
                modes_w=modes_w, Cm_w=Cm_w, Cm=Cm, tau=ired_mode_tau(Cm, dt), Ct_vec=np.ascontiguousarray(Ct_vec.reshape(shape).T),
                dCt_vec=np.ascontiguousarray(dCt_vec.reshape(shape).T))


def calculate_iRED(vec_list, dt, window=None, tau=None, n_global=5, ctx=None, mode_ct=False, n_lags=None):
    """iRED of a list of (frames, N, 3) float32 arrays, one per trajectory file (lab frame or superposed: M does not change
    under a rotation of a whole frame).  Uploads the vectors once; result (and mode_ct, n_lags) as calculate_iRED_resident."""
    vec_list = [np.ascontiguousarray(v, dtype=np.float32) for v in vec_list]
    for v in vec_list:
        if v.ndim != 3 or v.shape[2] != 3 or v.shape[1] != vec_list[0].shape[1]:
            raise ValueError('iRED: every file must be (frames, N, 3) with the same N')
    N = vec_list[0].shape[1]
    if N <= n_global:
        raise ValueError('iRED: %d vectors do not exceed the %d global modes' % (N, n_global))
    frames = [v.shape[0] for v in vec_list]
    with _ctx(ctx).vectors(N, sum(frames)) as rv:
        for v in vec_list:
            if v.shape[0] > 0:
                rv.append(v)
        return calculate_iRED_resident(rv, frames, dt, window=window, tau=tau, n_global=n_global, mode_ct=mode_ct, n_lags=n_lags)
