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

M, the one loop that is quadratic in the number of vectors, is computed on the MI355X (csrc/sr_ired.hip) and nowhere else: there
is no CPU path for it, without a GPU the calls raise SpinRelaxHipError.  The eigen-decomposition of the (N, N) matrices is
numpy.linalg.eigh on the host.
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


def calculate_iRED_resident(rv, frames_per_file, dt, window=None, tau=None, n_global=5):
    """iRED of resident vectors (hip.ResidentVectors) that hold the files one after the other, frames_per_file frames of each.
    Returns a dict: S2, dS2 (N), eig (N) = the eigenvalues averaged over the windows per rank, S2_w, lam_w (W, N), M (W, N, N),
    win_start, win_len."""
    if rv.nV <= n_global:
        raise ValueError('iRED: %d vectors do not exceed the %d global modes' % (rv.nV, n_global))
    win_start, win_len = ired_windows(frames_per_file, dt, window=window, tau=tau)
    if win_start.size < 1:
        raise ValueError('iRED: no file holds a whole window')
    return _analyse(rv.ired(win_start, win_len), win_start, win_len, n_global)


def calculate_iRED(vec_list, dt, window=None, tau=None, n_global=5, ctx=None):
    """iRED of a list of (frames, N, 3) float32 arrays, one per trajectory file (lab frame or superposed: M does not change
    under a rotation of a whole frame).  Uploads the vectors once; result as calculate_iRED_resident."""
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
        return calculate_iRED_resident(rv, frames, dt, window=window, tau=tau, n_global=n_global)
