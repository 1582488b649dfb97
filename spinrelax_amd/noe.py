"""
All-pairs dipolar map: effective distances and order parameters of EVERY pair of a set of spins, the screening step in front of the
distance-weighted correlation functions (ct.calculate_Ct_dipolar), which need their pairs named in advance.

With d = x_j - x_i in the molecule-fixed frame and r = |d|, per pair (Brueschweiler et al., J. Am. Chem. Soc. 114, 2289 (1992);
Peter, Daura & van Gunsteren, J. Biomol. NMR 20, 297 (2001)):

    A6   = <r^-6>                 reff6 = A6^(-1/6)      (fast-motion effective distance)
    A3   = <r^-3>                 reff3 = A3^(-1/3)      (slow-motion effective distance)
    T_ab = <d_a d_b r^-5>         (symmetric 3 x 3, tr T = A3)
    S2    = 1.5 (sum_ab T_ab^2 - A3^2 / 3) / A6          (the plateau of C_dd(k) as calculate_Ct_dipolar normalises it:
                                                          P2(u . u') = 1.5 Q : Q' with Q = u u - 1/3)
    S2rad = A3^2 / A6                                    (the radial order parameter calculate_Ct_dipolar returns)

The block sums of r^-6 and d_a d_b r^-5, the loop that is quadratic in the number of spins, are computed on the MI355X
(csrc/sr_noe.hip) and nowhere else: without a GPU dipolar_map raises SpinRelaxHipError.  Everything after the sums is finalize(),
pure numpy.

With lags (dipolar_map(..., lags=...)) the map also holds the dipolar correlation function of every pair at those lags,

    Cdd(k) = <P2(u(t) . u(t + k)) r(t)^-3 r(t + k)^-3> / A6       (calculate_Ct_dipolar's normalisation: Cdd(0) = 1, plateau S2)

from the block sums G_b(k) of csrc/sr_noe.hip, and from it the internal correlation time of the pair, the Lipari-Szabo integral
tau_e = int (Cdd - S2) / (1 - S2) dt (tau_e_from_Cdd): what noesy.rate_matrix(..., tau_e='map') takes.  finalize_lagged() is pure numpy.

With modes=True (dipolar_map(..., modes=True, frame=q_F)) the map also holds the split of A6 Cdd(k) into the five tumbling modes of an
anisotropic rotational diffusion tensor D = (Dx, Dy, Dz), whose principal-axis frame the constant unit quaternion q_F rotates into:
the six sums H of csrc/sr_noe.hip, which do not depend on D, and from them, host numpy,

    g_m(k), m = 0 .. 4   (mode_amplitudes(H[k], D): sum_m g_m(k) = A6 Cdd(k); rates E_m = _hostmath.D_coefficients_ellipsoid(D))
    c_m                  (mode_plateau(T, D, q_F): the plateau of g_m, from the map's mean tensor; sum_m c_m = S2 A6)
    tau_e per mode       (mode_tau_e(result, D): tau_e_from_Cdd of g_m(k) / g_m(0) with the plateau c_m / g_m(0))

what noesy.rate_matrix(..., D=...) takes.
"""
import warnings

import numpy as np

from . import hip
from ._hostmath import ellipsoid_R
from .ired import ired_reduce

# the seven sums per block and pair, in the library's order
COMPONENTS = ('r-6', 'xx', 'yy', 'zz', 'xy', 'xz', 'yz')


def _ctx(ctx):
    return ctx if ctx is not None else hip.default_context()


def n_pairs(P):
    return P * (P - 1) // 2


def pair_index(i, j, P):
    """position of the pair i < j (positions in the index list of P atoms) in the library's order, row-major over i < j:
    k = i (2 P - i - 1) / 2 + (j - i - 1); arrays broadcast"""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    if np.any(i < 0) or np.any(j <= i) or np.any(j >= P):
        raise ValueError('pair_index needs 0 <= i < j < P')
    return i * (2 * P - i - 1) // 2 + (j - i - 1)


def pair_list(P):
    """(P (P - 1) / 2, 2) int64: the pairs (i, j) in the library's order, the inverse of pair_index"""
    k = np.arange(n_pairs(P), dtype=np.int64)
    # row i starts at i (2 P - i - 1) / 2: the largest i with that start <= k
    i = np.floor(((2 * P - 1) - np.sqrt((2.0 * P - 1) ** 2 - 8.0 * k)) / 2).astype(np.int64)
    i -= (i * (2 * P - i - 1) // 2 > k)                   # the square root may round across a row start, either way
    i += ((i + 1) * (2 * P - i - 2) // 2 <= k)
    j = k - i * (2 * P - i - 1) // 2 + i + 1
    return np.stack([i, j], axis=1)


def _tensor(s):
    """sums or averages (..., 7) -> (..., 3, 3)"""
    T = np.empty(s.shape[:-1] + (3, 3))
    T[..., 0, 0], T[..., 1, 1], T[..., 2, 2] = s[..., 1], s[..., 2], s[..., 3]
    T[..., 0, 1] = T[..., 1, 0] = s[..., 4]
    T[..., 0, 2] = T[..., 2, 0] = s[..., 5]
    T[..., 1, 2] = T[..., 2, 1] = s[..., 6]
    return T


def _derive(avg):
    """averages (..., 7) -> A6, A3, T, reff6, reff3, S2, S2rad"""
    A6 = avg[..., 0]
    T = _tensor(avg)
    A3 = avg[..., 1] + avg[..., 2] + avg[..., 3]
    TT = np.einsum('...ab,...ab->...', T, T)
    return A6, A3, T, A6 ** (-1.0 / 6.0), A3 ** (-1.0 / 3.0), 1.5 * (TT - A3 * A3 / 3.0) / A6, A3 * A3 / A6


def _error(v_b):
    """per-block values (B, n) -> their error by the convention of ired.ired_reduce: std(ddof = 0) / (sqrt(B) - 1), 0 for B = 1"""
    return ired_reduce(v_b)[1]


def finalize(sums, block_len):
    """sums (B, npairs, 7) float64 as the library writes them, block_len (B) frames per block -> dict:
      A6, A3 (npairs), T (npairs, 3, 3), reff6, reff3, S2, S2rad (npairs) from the sums over ALL blocks (S2 is not linear in the
        averages: totals, not the mean of the block values);
      dS2, dreff6, dreff3 (npairs) from the per-block values, std(ddof = 0) / (sqrt(B) - 1) like ired.ired_reduce, 0 for one block;
      A6_b, A3_b, reff6_b, reff3_b, S2_b, S2rad_b (B, npairs) and T_b (B, npairs, 3, 3), the per-block values; block_len.
    A non-finite sum means that two of the atoms coincided in some frame: ValueError, naming the first such pair."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 3 or sums.shape[2] != 7:
        raise ValueError('sums must be (blocks, pairs, 7), got %s' % (sums.shape,))
    bl = np.atleast_1d(np.asarray(block_len, dtype=np.int64))
    if bl.shape != (sums.shape[0],) or np.any(bl < 1):
        raise ValueError('block_len must give one length >= 1 per block')
    bad = np.nonzero(~np.isfinite(sums).all(axis=(0, 2)))[0]
    if bad.size:
        # P from npairs = P (P - 1) / 2
        P = int(round((1 + np.sqrt(1.0 + 8.0 * sums.shape[1])) / 2))
        i, j = pair_list(P)[bad[0]]
        raise ValueError('dipolar map: the sums of pair %d (positions %d and %d of the index list) are not finite: the two atoms '
                         'coincide in some frame' % (bad[0], i, j))
    A6, A3, T, reff6, reff3, S2, S2rad = _derive(sums.sum(axis=0) / float(bl.sum()))
    A6_b, A3_b, T_b, reff6_b, reff3_b, S2_b, S2rad_b = _derive(sums / bl[:, None, None].astype(np.float64))
    return dict(A6=A6, A3=A3, T=T, reff6=reff6, reff3=reff3, S2=S2, S2rad=S2rad,
                dS2=_error(S2_b), dreff6=_error(reff6_b), dreff3=_error(reff3_b),
                A6_b=A6_b, A3_b=A3_b, T_b=T_b, reff6_b=reff6_b, reff3_b=reff3_b, S2_b=S2_b, S2rad_b=S2rad_b, block_len=bl)


def _blocks(blocks, n_frames):
    """None -> one block of all frames; otherwise (block_start, block_len)"""
    if blocks is None:
        return np.zeros(1, dtype=np.int64), np.full(1, n_frames, dtype=np.int64)
    bs, bl = blocks
    return np.ascontiguousarray(np.atleast_1d(bs), dtype=np.int64), np.ascontiguousarray(np.atleast_1d(bl), dtype=np.int64)


def log_lags(max_lag, n):
    """about n integer lags from 1 to max_lag, log-spaced, rounded and deduplicated: strictly increasing int64, the first 1, the last
    max_lag (fewer than n where the rounding merges neighbours, all of 1 .. max_lag when n >= max_lag)"""
    max_lag, n = int(max_lag), int(n)
    if max_lag < 1 or n < 1 or (n < 2 and max_lag > 1):
        raise ValueError('log_lags needs max_lag >= 1 and n >= 2 lags (one lag only for max_lag = 1)')
    lags = np.unique(np.rint(np.geomspace(1.0, float(max_lag), n)).astype(np.int64))
    lags[0], lags[-1] = 1, max_lag
    return np.unique(lags)


def _lag_array(lags):
    lg = np.atleast_1d(np.asarray(lags))
    if lg.ndim != 1 or lg.size < 1 or lg.dtype.kind not in 'iu':
        raise ValueError('lags must be a non-empty 1-D list of integers')
    return lg.astype(np.int64)


def tau_e_from_Cdd(Cdd, S2, lags, dt=1.0):
    """The internal correlation time of Lipari & Szabo, tau_e = int_0^inf (C(t) - S2) / (1 - S2) dt, from C at a few lags: Cdd (K, n)
    (or (K) for one series), S2 (n), lags (K) strictly increasing, in frames of dt -> tau_e (n) in the units of dt.  The trapezoid rule
    through (0, 1) and the given points (a given lag 0 is replaced by that point); the integral stops at the first point with
    C <= S2, the crossing located by linear interpolation; 0 where 1 - S2 < 1e-6 (a rigid pair has no internal term)."""
    lg = _lag_array(lags)
    C = np.asarray(Cdd, dtype=np.float64)
    one = C.ndim == 1
    C = C.reshape(lg.size, -1) if one else C
    S2 = np.atleast_1d(np.asarray(S2, dtype=np.float64))
    if C.ndim != 2 or C.shape[0] != lg.size or S2.shape != (C.shape[1],):
        raise ValueError('tau_e_from_Cdd needs Cdd (lags, n) and S2 (n)')
    if np.any(lg < 0) or np.any(np.diff(lg) <= 0):
        raise ValueError('lags must be >= 0 and strictly increasing')
    if lg[0] == 0:
        lg, C = lg[1:], C[1:]
    flex = (1.0 - S2) >= 1e-6
    den = np.where(flex, 1.0 - S2, 1.0)
    t = np.concatenate([[0.0], lg.astype(np.float64)])          # in frames: dt multiplies the finished integral, exactly linear in it
    Y = np.concatenate([np.ones((1, C.shape[1])), (C - S2[None]) / den[None]], axis=0)
    alive = np.logical_and.accumulate(Y > 0, axis=0)           # up to and including this point the series stayed above S2
    tau = np.zeros(C.shape[1])
    for k in range(1, t.size):
        h = t[k] - t[k - 1]
        y0, y1 = Y[k - 1], Y[k]
        with np.errstate(divide='ignore', invalid='ignore'):
            cross = 0.5 * y0 * y0 / (y0 - y1) * h              # the triangle up to the crossing at t[k-1] + h y0 / (y0 - y1)
        tau += np.where(alive[k], 0.5 * (y0 + y1) * h, np.where(alive[k - 1], cross, 0.0))
    tau = np.where(flex, tau, 0.0) * float(dt)
    return float(tau[0]) if one else tau


def finalize_lagged(G, block_len, lags, fin, dt=1.0):
    """G (B, K, npairs) float64 as the library writes it, block_len (B), lags (K) and fin = finalize()'s dict of the same blocks ->
    dict: lags (K) int64, G, Cdd (K, npairs) = [sum_b G_b(k) / sum_b (n_b - k)] / A6 (for blocks of equal length
    calculate_Ct_dipolar's normalisation), dCdd (K, npairs) from the per-block values G_b(k) / (n_b - k) / A6_b by the convention of
    ired.ired_reduce, tau_e (npairs) = tau_e_from_Cdd(Cdd, S2, lags, dt) in the units of dt, dtau_e from the per-block values, each
    with its block's own S2_b; Cdd_b (B, K, npairs), tau_e_b (B, npairs) and dt."""
    G = np.asarray(G, dtype=np.float64)
    lg = _lag_array(lags)
    bl = np.atleast_1d(np.asarray(block_len, dtype=np.int64))
    if G.ndim != 3 or G.shape[:2] != (bl.size, lg.size) or G.shape[2] != fin['A6'].size:
        raise ValueError('G must be (blocks, lags, pairs), got %s' % (G.shape,))
    terms = bl[:, None] - lg[None, :]                           # (B, K) origins per block and lag
    if np.any(terms < 1):
        raise ValueError('every lag must leave a term in every block')
    Cdd = G.sum(axis=0) / terms.sum(axis=0)[:, None].astype(np.float64) / fin['A6'][None]
    Cdd_b = G / terms[:, :, None].astype(np.float64) / fin['A6_b'][:, None, :]
    tau_e = tau_e_from_Cdd(Cdd, fin['S2'], lg, dt)
    tau_e_b = np.stack([tau_e_from_Cdd(Cdd_b[b], fin['S2_b'][b], lg, dt) for b in range(bl.size)])
    return dict(lags=lg, dt=float(dt), G=G, Cdd=Cdd, dCdd=_error(Cdd_b.reshape(bl.size, -1)).reshape(Cdd.shape), tau_e=tau_e, dtau_e=_error(tau_e_b),
                Cdd_b=Cdd_b, tau_e_b=tau_e_b)


def _frame_quat(frame):
    """None, or the unit quaternion (w, x, y, z) as float64 (4); ValueError for anything else"""
    if frame is None:
        return None
    q = np.asarray(frame, dtype=np.float64)
    if q.shape != (4,) or not np.all(np.isfinite(q)) or abs(float(q @ q) - 1.0) > 1e-6:
        raise ValueError('frame must be a unit quaternion (w, x, y, z)')
    return q


def frame_matrix(frame):
    """R(q_F) (3, 3) of the frame quaternion (normalised), the identity for None: v' = R v is --vecRot's q v q*"""
    q = _frame_quat(frame)
    if q is None:
        return np.eye(3)
    w, x, y, z = q / np.sqrt(q @ q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _tensor_D(D):
    D = np.asarray(D, dtype=np.float64)
    if D.shape != (3,) or not np.all(np.isfinite(D)) or np.any(D <= 0):
        raise ValueError('D must be (Dx, Dy, Dz), finite and > 0')
    return D


def mode_amplitudes(H, D):
    """The six mode sums H (..., 6) of csrc/sr_noe.hip (sums or averages: the map is linear) -> the amplitudes (..., 5) of the five
    rates of D = (Dx, Dy, Dz), in the order of _hostmath.D_coefficients_ellipsoid:
        g_0 = 3 H3, g_1 = 3 H4, g_2 = 3 H5, g_3 = dd - e, g_4 = dd + e,   dd = 1.125 H0 + 0.375 H1,
        e = sum_i c_i (3 <q_i q'_i> + 6 sym<q_j q'_k>),   c_i = (D_i - Diso) / (12 R), 0 for the sphere (_hostmath.A_coefficients_ellipsoid),
    q_i = u_i^2 - 1/3, so that with qz = q_z and dl = q_x - q_y: <q_x q'_x> = (H0 - 2 H2 + H1) / 4, <q_y q'_y> = (H0 + 2 H2 + H1) / 4,
    <q_z q'_z> = H0, sym<q_x q'_y> = (H0 - H1) / 4, sym<q_x q'_z> = (H2 - H0) / 2, sym<q_y q'_z> = -(H0 + H2) / 2.
    Their sum is 2.25 H0 + 0.75 H1 + 3 (H3 + H4 + H5) = sum w P2(u . v), the lagged map's G.  For H of one unit vector (u = v, w = 1)
    they are A_coefficients_ellipsoid(u, D)."""
    H = np.asarray(H, dtype=np.float64)
    if H.shape[-1] != 6:
        raise ValueError('H must be (..., 6), got %s' % (H.shape,))
    D = _tensor_D(D)
    R = float(ellipsoid_R(D))
    s = 1.0 / (12.0 * R) if R > 0.0 else 0.0
    cx, cy, cz = (D - D.mean()) * s
    H0, H1, H2, H3, H4, H5 = (H[..., k] for k in range(6))
    xx, yy, zz = 0.25 * (H0 - 2.0 * H2 + H1), 0.25 * (H0 + 2.0 * H2 + H1), H0
    xy, xz, yz = 0.25 * (H0 - H1), 0.5 * (H2 - H0), -0.5 * (H0 + H2)
    dd = 1.125 * H0 + 0.375 * H1
    e = cx * (3.0 * xx + 6.0 * yz) + cy * (3.0 * yy + 6.0 * xz) + cz * (3.0 * zz + 6.0 * xy)
    return np.stack((3.0 * H3, 3.0 * H4, 3.0 * H5, dd - e, dd + e), axis=-1)


def mode_plateau(T, D, frame=None):
    """The plateaus c_m (..., 5) of the mode functions from the map's mean tensor T (..., 3, 3) = <d d^T r^-5> (in the frame the map
    was made in) and the frame quaternion: Qbar = F T F^T - (tr T / 3) 1, F = R(frame), and mode_amplitudes of H0 = Qbar_zz^2,
    H1 = (Qbar_xx - Qbar_yy)^2, H2 = Qbar_zz (Qbar_xx - Qbar_yy), H3 = Qbar_yz^2, H4 = Qbar_xz^2, H5 = Qbar_xy^2.  sum_m c_m = S2 A6."""
    T = np.asarray(T, dtype=np.float64)
    if T.shape[-2:] != (3, 3):
        raise ValueError('T must be (..., 3, 3), got %s' % (T.shape,))
    F = frame_matrix(frame)
    Q = np.einsum('ab,...bc,dc->...ad', F, T, F)
    tr = (Q[..., 0, 0] + Q[..., 1, 1] + Q[..., 2, 2]) / 3.0
    qz, dl = Q[..., 2, 2] - tr, Q[..., 0, 0] - Q[..., 1, 1]
    H = np.stack((qz * qz, dl * dl, qz * dl, Q[..., 1, 2] ** 2, Q[..., 0, 2] ** 2, Q[..., 0, 1] ** 2), axis=-1)
    return mode_amplitudes(H, D)


def mode_tau_e(result, D):
    """The internal correlation time of every pair and mode (npairs, 5), in the units of the map's dt, of a map made with modes=True and
    lags beyond 0: tau_e_from_Cdd of g_m(k) / a_m with the plateau c_m / a_m, a_m = g_m(0), c_m = mode_plateau(T, D, frame); 0 for a
    mode whose a_m - c_m is not positive (no decay to describe)."""
    if 'H' not in result:
        raise ValueError('mode_tau_e needs a map made with modes=True (noe.dipolar_map(..., modes=True)): this one holds no H')
    lg = np.asarray(result['lags'], dtype=np.int64)
    if lg.size < 2:
        raise ValueError('mode_tau_e needs a map with lags beyond 0 (noe.dipolar_map(..., modes=True, lags=[0, ...]))')
    g = mode_amplitudes(result['H'], D)                          # (K, npairs, 5)
    c = mode_plateau(result['T'], D, result.get('frame'))
    a = g[0]
    live = (a > 0) & (a - c > 0)
    den = np.where(live, a, 1.0)
    C = np.where(live[None], g / den[None], 1.0).reshape(lg.size, -1)
    S2 = np.where(live, np.clip(c, 0.0, None) / den, 1.0).reshape(-1)
    return tau_e_from_Cdd(C, S2, lg, float(result.get('dt', 1.0))).reshape(a.shape)


def finalize_modes(Hb, block_len, lags, frame=None):
    """H_blocks (B, K, npairs, 6) float64 as the library writes it, block_len (B), lags (K) starting at 0 -> dict: H (K, npairs, 6) =
    sum_b H_b(k) / sum_b (n_b - k), the average over the origins; H_blocks; frame (the quaternion, (1, 0, 0, 0) for None)"""
    Hb = np.asarray(Hb, dtype=np.float64)
    lg = _lag_array(lags)
    bl = np.atleast_1d(np.asarray(block_len, dtype=np.int64))
    if Hb.ndim != 4 or Hb.shape[:2] != (bl.size, lg.size) or Hb.shape[3] != 6:
        raise ValueError('H_blocks must be (blocks, lags, pairs, 6), got %s' % (Hb.shape,))
    terms = bl[:, None] - lg[None, :]
    if np.any(terms < 1):
        raise ValueError('every lag must leave a term in every block')
    q = _frame_quat(frame)
    return dict(H=Hb.sum(axis=0) / terms.sum(axis=0)[:, None, None].astype(np.float64), H_blocks=Hb,
                frame=np.array([1.0, 0.0, 0.0, 0.0]) if q is None else q)


def _mode_lags(lags, modes, frame):
    """the lag list of a map with modes (None -> [0]; it must start at 0: a_m is the lag-0 value) and the checked frame quaternion;
    ValueError before a context is asked for"""
    if not modes:
        if frame is not None:
            raise ValueError('frame belongs to modes=True')
        return (None if lags is None else _lag_array(lags)), None
    lg = np.zeros(1, dtype=np.int64) if lags is None else _lag_array(lags)
    if lg[0] != 0:
        raise ValueError('a map with modes=True needs lags that start at 0 (the mode amplitudes a_m are the lag-0 values), got %d' % lg[0])
    return lg, _frame_quat(frame)


def _result(sums, bl, index, G=None, lags=None, dt=1.0, Hb=None, mode_lags=None, frame=None):
    index = np.asarray(index)
    out = finalize(sums, bl)
    out['pairs'] = pair_list(index.size)
    out['index'] = index.astype(np.int64)
    out['sums'] = sums
    if G is not None:
        out.update(finalize_lagged(G, bl, lags, out, dt))
    if Hb is not None:
        out.update(finalize_modes(Hb, bl, mode_lags, frame))
        out.setdefault('lags', mode_lags)
        out.setdefault('dt', float(dt))
    return out


def dipolar_map(xyz, index, quat=None, blocks=None, mode=0, ctx=None, lags=None, dt=1.0, modes=False, frame=None):
    """The map of every pair of the atoms `index` of the coordinates xyz (frames, atoms, 3) float32.  quat (frames, 4) float64: the
    unit quaternion (w, x, y, z) that takes each frame into the molecule-fixed frame (what ct.superpose_XHvecs(..., want_quat=True)
    returns); None: the lab frame, S2 then includes overall tumbling.  blocks = (block_start, block_len) in frames (ragged lengths
    allowed), None: one block.  mode 0: float32 per pair and frame, 1: float64 throughout.
    Returns finalize()'s dict and pairs (npairs, 2) positions in `index`, index, sums (B, npairs, 7).
    lags: integer lags in frames (strictly increasing, >= 0, below the shortest block, at most 64; log_lags makes such a list), dt the
    time between frames: the dict then also holds finalize_lagged()'s lags, G, Cdd, dCdd, tau_e, dtau_e (tau_e in the units of dt).
    None: the map alone, as ever.
    modes=True: also the mode sums of csrc/sr_noe.hip for anisotropic tumbling, in the frame R(frame) R(quat[t]); frame: the
    constant unit quaternion (w, x, y, z) from the molecule-fixed frame into the diffusion tensor's principal-axis frame (--vecRot's
    convention), None: identity.  The lags must start at 0 (None: [0]; ValueError otherwise, before a context is asked for).  The
    dict then also holds finalize_modes()'s H (K, npairs, 6), H_blocks (B, K, npairs, 6) and frame, with lags and dt."""
    lg, fq = _mode_lags(lags, modes, frame)
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    bs, bl = _blocks(blocks, xyz.shape[0])
    c = _ctx(ctx)
    if lg is None:
        return _result(c.noe_pairs(xyz, index, quat=quat, block_start=bs, block_len=bl, mode=mode), bl, index)
    if xyz.ndim == 3:
        if lags is not None:
            c.noe_lagged_check(xyz.shape[0], xyz.shape[1], index, bs, bl, lg, mode)     # the lags' refusals before the map is computed
        if modes:
            c.noe_modes_check(xyz.shape[0], xyz.shape[1], index, bs, bl, lg, frame=fq, mode=mode)
    sums = c.noe_pairs(xyz, index, quat=quat, block_start=bs, block_len=bl, mode=mode)
    G = c.noe_lagged(xyz, index, lg, quat=quat, block_start=bs, block_len=bl, mode=mode) if lags is not None else None
    Hb = c.noe_modes(xyz, index, lg, quat=quat, frame=fq, block_start=bs, block_len=bl, mode=mode) if modes else None
    return _result(sums, bl, index, G, lg, dt, Hb, lg, fq)


def dipolar_map_superposed(xyz, ref_xyz, fit_indices, index, blocks=None, mode=0, ctx=None, lags=None, dt=1.0, modes=False, frame=None):
    """dipolar_map in the frame of the per-frame least-squares superposition onto ref_xyz (atoms, 3) over fit_indices, the front end's
    (Context.xh_vectors / ct.superpose_XHvecs): the coordinates are uploaded once, the front end's kernel leaves its quaternions on
    the device and the map reads them there.  The result also holds quat (frames, 4).  lags, dt, modes, frame: as in dipolar_map; the
    lagged and the mode sums read the same device coordinates and quaternions."""
    import torch
    mlg, fq = _mode_lags(lags, modes, frame)
    c = _ctx(ctx)
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    if xyz.ndim != 3 or xyz.shape[2] != 3:
        raise ValueError('xyz must be (frames, atoms, 3)')
    nF, nA, _ = xyz.shape
    index = np.asarray(index)
    bs, bl = _blocks(blocks, nF)
    c.noe_pairs_check(nF, nA, index, bs, bl, mode)  # the library's refusals, a map beyond the device's memory among them, before torch allocates
    lg = None if lags is None else _lag_array(lags)
    if lg is not None:
        c.noe_lagged_check(nF, nA, index, bs, bl, lg, mode)
    if modes:
        c.noe_modes_check(nF, nA, index, bs, bl, mlg, frame=fq, mode=mode)
    dev = torch.device('cuda', c.device)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)    # a read-only array: it is only read
        xyz_d = torch.from_numpy(xyz).to(dev)
    quat_d = torch.empty((nF, 4), dtype=torch.float64, device=dev)
    sums_d = torch.empty((bs.size, n_pairs(index.size), 7), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)                     # the upload is torch's, the kernels run on the context's stream
    c.xh_quat_dev(xyz_d.data_ptr(), nF, nA, fit_indices, ref_xyz, quat_d.data_ptr())
    c.noe_pairs_dev(xyz_d.data_ptr(), nF, nA, index, quat_d.data_ptr(), bs, bl, sums_d.data_ptr(), mode=mode)
    G_d = None
    if lg is not None:
        G_d = torch.empty((bs.size, lg.size, n_pairs(index.size)), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        c.noe_lagged_dev(xyz_d.data_ptr(), nF, nA, index, quat_d.data_ptr(), bs, bl, lg, G_d.data_ptr(), mode=mode)
    H_d = None
    if modes:
        H_d = torch.empty((bs.size, mlg.size, n_pairs(index.size), 6), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        c.noe_modes_dev(xyz_d.data_ptr(), nF, nA, index, quat_d.data_ptr(), bs, bl, mlg, H_d.data_ptr(), frame=fq, mode=mode)
    c.sync()
    out = _result(sums_d.cpu().numpy(), bl, index, None if G_d is None else G_d.cpu().numpy(), lg, dt,
                  None if H_d is None else H_d.cpu().numpy(), mlg, fq)
    out['quat'] = quat_d.cpu().numpy()
    return out


def select_pairs(result, cutoff):
    """The pairs of a map with reff6 <= cutoff (units of the coordinates) as (indexX, indexH): ATOM indices, int64, in the form
    ct.superpose_XHvecs takes -- their vectors then go to ct.calculate_Ct_dipolar."""
    keep = np.nonzero(result['reff6'] <= cutoff)[0]
    pr = result['pairs'][keep]
    idx = np.asarray(result['index'], dtype=np.int64)
    return idx[pr[:, 0]], idx[pr[:, 1]]


COLUMNS = ('i', 'j', 'name_i', 'name_j', 'reff6', 'dreff6', 'reff3', 'S2', 'dS2', 'S2rad')


def _rows(result, names, cutoff):
    """what write_map and write_map_ct share: the atom indices, one checked name per atom, the pairs the cutoff keeps"""
    idx = np.asarray(result['index'], dtype=np.int64)
    names = [str(a) for a in idx] if names is None else [str(n) for n in names]
    if len(names) != idx.size:
        raise ValueError('names must give one name per selected atom')
    if any((not n) or any(ch.isspace() for ch in n) for n in names):
        raise ValueError('names must be non-empty and free of white space')
    keep = np.arange(result['reff6'].size) if cutoff is None else np.nonzero(result['reff6'] <= cutoff)[0]
    return idx, names, keep


def write_map(path, result, names=None, cutoff=None):
    """<o>_noeMap.dat: one row per pair, columns i j name_i name_j reff6 dreff6 reff3 S2 dS2 S2rad (i, j atom indices, the numbers
    as %.8g); cutoff keeps the pairs with reff6 <= cutoff.  names: one per entry of the index list, default the atom index.
    Returns the number of rows."""
    idx, names, keep = _rows(result, names, cutoff)
    with open(path, 'w') as fp:
        fp.write('# ' + ' '.join(COLUMNS) + '\n')
        for k in keep:
            i, j = result['pairs'][k]
            fp.write('%d %d %s %s %s\n' % (idx[i], idx[j], names[i], names[j], ' '.join(
                '%.8g' % result[c][k] for c in COLUMNS[4:])))
    return int(keep.size)


def read_map(path):
    """parse write_map's file back: dict of arrays, i and j int64, the names as lists of str, the rest float64"""
    cols = {c: [] for c in COLUMNS}
    with open(path) as fp:
        for line in fp:
            if line.startswith('#') or not line.strip():
                continue
            w = line.split()
            if len(w) != len(COLUMNS):
                raise ValueError('%s: a row with %d columns, expected %d' % (path, len(w), len(COLUMNS)))
            for c, v in zip(COLUMNS, w):
                cols[c].append(v)
    out = {}
    for c in COLUMNS:
        if c in ('i', 'j'):
            out[c] = np.array(cols[c], dtype=np.int64)
        elif c.startswith('name'):
            out[c] = cols[c]
        else:
            out[c] = np.array(cols[c], dtype=np.float64)
    return out


def _ct_columns(lags, dt):
    return ['i', 'j', 'name_i', 'name_j', 'tau_e', 'dtau_e'] + ['Cdd(%.8g)' % (k * dt) for k in lags]


def write_map_ct(path, result, names=None, cutoff=None):
    """<o>_noeMapCt.dat of a map with lags: a header '# i j name_i name_j tau_e dtau_e Cdd(t0) Cdd(t1) ...', a line '# lags t0 t1 ...'
    (the lags in time units, lag x the map's dt, %.8g), then one row per pair: the atom indices, the names, tau_e and dtau_e (in the units the
    map was made with) and one Cdd column per lag, %.8g.  names and cutoff as in write_map.  Returns the number of rows."""
    if 'Cdd' not in result:
        raise ValueError('write_map_ct needs a map with lags (dipolar_map(..., lags=...))')
    idx, names, keep = _rows(result, names, cutoff)
    lags, dt = np.asarray(result['lags'], dtype=np.int64), float(result.get('dt', 1.0))
    with open(path, 'w') as fp:
        fp.write('# ' + ' '.join(_ct_columns(lags, dt)) + '\n')
        fp.write('# lags ' + ' '.join('%.8g' % (k * dt) for k in lags) + '\n')
        for k in keep:
            i, j = result['pairs'][k]
            fp.write('%d %d %s %s %.8g %.8g %s\n' % (idx[i], idx[j], names[i], names[j], result['tau_e'][k], result['dtau_e'][k],
                                                     ' '.join('%.8g' % v for v in result['Cdd'][:, k])))
    return int(keep.size)


def read_map_ct(path):
    """parse write_map_ct's file back: dict(i, j int64, name_i, name_j lists of str, tau_e, dtau_e (rows) float64, Cdd (rows, K)
    float64, lags (K) float64 in time units)"""
    lags = None
    i, j, ni, nj, te, dte, C = [], [], [], [], [], [], []
    with open(path) as fp:
        for line in fp:
            if line.startswith('# lags'):
                lags = np.array(line.split()[2:], dtype=np.float64)
                continue
            if line.startswith('#') or not line.strip():
                continue
            w = line.split()
            if lags is None or len(w) != 6 + lags.size:
                raise ValueError('%s: a row with %d columns, expected %s' % (path, len(w), 'a lags line first' if lags is None else 6 + lags.size))
            i.append(w[0]); j.append(w[1]); ni.append(w[2]); nj.append(w[3]); te.append(w[4]); dte.append(w[5]); C.append(w[6:])
    if lags is None:
        raise ValueError('%s: no lags line' % path)
    return dict(i=np.array(i, dtype=np.int64), j=np.array(j, dtype=np.int64), name_i=ni, name_j=nj, tau_e=np.array(te, dtype=np.float64),
                dtau_e=np.array(dte, dtype=np.float64), Cdd=np.array(C, dtype=np.float64).reshape(len(i), lags.size), lags=lags)
