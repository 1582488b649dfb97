"""
Relaxation of a bond vector under anisotropic tumbling from its mode-resolved correlation function (ct.calculate_Ct_modes,
csrc/sr_ct_modes.hip), an extension beyond the reference.  Host numpy only: the hot path is the kernel that makes H.

The reference's form for an axisymmetric or rhombic tensor takes a static histogram of the vector's orientation in the principal-axis
frame and multiplies it by ONE internal C(t) shared by the five modes, J(w) = sum_m <A_m>_hist FT[C_I(t) exp(-E_m t)]: exact only if
the internal motion decays every mode alike.  Here every mode has its own function.  With the six sums H(k) of the five signals
(include/spinrelax_hip.h), a_m(k) = noe.mode_amplitudes(H(k), D) is the correlation function of mode m, a_m(0) its amplitude (for a
rigid vector A_coefficients_ellipsoid(u, D)), c_m = noe.mode_amplitudes of the products of the mean signals its plateau, E_m the five
rates of _hostmath.D_coefficients_ellipsoid, and with no further assumption than the independence of internal motion and tumbling

    J(w) = sum_m [ c_m g(E_m, w) + Re int_0^T (a_m(t) - c_m) exp(-(E_m + i w) t) dt ],     g(x, y) = x / (x^2 + y^2)

the integral taken exactly for the piecewise-linear interpolant of the samples (pl_transform).  sum_m a_m(k) is C(k) of kernel 1 and
sum_m c_m the order parameter S2.  For the sphere D = (1, 1, 1) / (6 tau_c) all five rates are 1 / tau_c and J is the isotropic one.

Errors of a_m, J and the rates need chunk-resolved sums (the error of a ratio or of an integral is not a function of dH alone) and are
not computed here.
"""
import numpy as np

from ._hostmath import D_coefficients_ellipsoid
from .noe import _tensor_D, mode_amplitudes


def _result_arrays(result):
    H = np.asarray(result['H'], dtype=np.float64)
    m = np.asarray(result['smean'], dtype=np.float64)
    if H.ndim != 3 or H.shape[2] != 6 or m.shape != (H.shape[1], 5):
        raise ValueError('result must hold H (lags, vectors, 6) and smean (vectors, 5) as ct.calculate_Ct_modes returns them')
    return H, m


def amplitudes(result, D):
    """result (the dict of ct.calculate_Ct_modes) and D = (Dx, Dy, Dz) in the frame the result was made in ->
    a (L + 1, nV, 5) the five mode functions at the lags 0 .. L, c (nV, 5) their plateaus, E (5) the rates of the modes."""
    H, m = _result_arrays(result)
    D = _tensor_D(D)
    Hp = np.stack((m[:, 0] ** 2, m[:, 1] ** 2, m[:, 0] * m[:, 1], m[:, 2] ** 2, m[:, 3] ** 2, m[:, 4] ** 2), axis=-1)
    return mode_amplitudes(H, D), mode_amplitudes(Hp, D), D_coefficients_ellipsoid(D)


def _psi(x):
    """psi(x) = (exp(-x) - 1 + x) / x^2 for complex x: the power series sum (-x)^n / (n + 2)! where |x| < 0.5 (the closed form cancels
    there), the closed form elsewhere"""
    x = np.asarray(x, dtype=np.complex128)
    small = np.abs(x) < 0.5
    xs = np.where(small, x, 0.0)
    series = np.zeros_like(xs)
    term = np.full_like(xs, 0.5)                 # n = 0: 1 / 2!
    for n in range(24):
        series = series + term
        term = term * (-xs) / (n + 3.0)
    xl = np.where(small, 1.0, x)
    return np.where(small, series, (np.exp(-xl) - 1.0 + xl) / (xl * xl))


def pl_transform(f, h, z):
    """int_0^((n-1) h) f~(t) exp(-z t) dt for the piecewise-linear interpolant f~ of the samples f[j] = f(j h), j < n (along axis 0),
    and complex z = E + i w: exact for f~, so the result does not depend on w h.  Interior nodes weigh h [sinh(z h / 2) / (z h / 2)]^2
    exp(-z t_j), the two end nodes h psi(+-z h), psi(x) = (exp(-x) - 1 + x) / x^2 (_psi).  The shapes of f behind axis 0 and of z
    broadcast; one sample gives 0 (an interval of no length)."""
    f = np.asarray(f, dtype=np.float64)
    z = np.asarray(z, dtype=np.complex128)
    if f.ndim < 1 or f.shape[0] < 1:
        raise ValueError('pl_transform needs at least one sample along axis 0')
    n = f.shape[0]
    nd = max(f.ndim - 1, z.ndim)
    f = f.reshape((n,) + (1,) * (nd - (f.ndim - 1)) + f.shape[1:])
    z = z.reshape((1,) * (nd - z.ndim) + z.shape)
    if n == 1:
        return np.zeros(np.broadcast_shapes(f.shape[1:], z.shape), dtype=np.complex128)
    x = z * float(h)
    y = 0.5 * x
    ys = np.where(y == 0, 1.0, y)
    interior = np.where(y == 0, 1.0, np.sinh(ys) / ys) ** 2
    j = np.arange(n, dtype=np.float64).reshape((n,) + (1,) * nd)
    w = np.exp(-x[None] * j) * interior[None]
    w[0] = _psi(x)
    w[n - 1] = np.exp(-x * (n - 1.0)) * _psi(-x)
    return float(h) * (f * w).sum(axis=0)


def _g(x, y):
    return x / (x * x + y * y)


def J(result, D, omega, dt, stop='crossing'):
    """The spectral density (nV, len(omega)) of every vector of `result` (ct.calculate_Ct_modes) tumbling with D = (Dx, Dy, Dz), in
    the units of dt: omega in rad per unit of dt, D in 1 / that unit.
        J(w) = sum_m [ c_m g(E_m, w) + Re pl_transform(a_m - c_m, dt, E_m + i w) ],   g(x, y) = x / (x^2 + y^2)
    stop = 'crossing': the integral of a mode ends where a_m first falls to c_m, at the crossing located by linear interpolation between
    the first lag with a_m(k) <= c_m and the one before it -- the rule of noe.tau_e_from_Cdd, which keeps the noise of a decayed
    function out of the integral; 'end': all L lags.  No error estimate: it needs chunk-resolved sums (the module's docstring)."""
    if stop not in ('crossing', 'end'):
        raise ValueError("stop must be 'crossing' or 'end'")
    a, c, E = amplitudes(result, D)
    om = np.atleast_1d(np.asarray(omega, dtype=np.float64))
    if om.ndim != 1:
        raise ValueError('omega must be a list of angular frequencies')
    if not (np.isfinite(dt) and dt > 0):
        raise ValueError('dt must be positive')
    nV = a.shape[1]
    out = np.zeros((nV, om.size))
    for v in range(nV):
        for m in range(5):
            z = E[m] + 1j * om
            y = a[:, v, m] - c[v, m]
            val = c[v, m] * _g(E[m], om)
            below = np.nonzero(y <= 0.0)[0] if stop == 'crossing' else ()
            if len(below) == 0:
                val = val + pl_transform(y, dt, z).real
            elif below[0] > 0:
                k = int(below[0])
                val = val + pl_transform(y[:k], dt, z).real
                hp = dt * y[k - 1] / (y[k - 1] - y[k])          # the last piece: from y[k - 1] down to 0 over hp
                val = val + (np.exp(-z * (k - 1) * dt) * y[k - 1] * hp * _psi(z * hp)).real
            out[v] += val
    return out


def relaxation(result, D, dt, field_MHz, nuclei='NH', time_unit='ps', rXH=None, csa=None, stop='crossing'):
    """R1, R2 and the heteronuclear NOE of the X-H pair of every vector from J above, with the constants and the rate formulas of the
    chain (spectral_densities.relaxationModel: get_f_DD, get_f_CSA, the five frequencies 0, wX, wH - wX, wH, wH + wX; the expressions
    of _obtain_R1R2NOErho) and its defaults for the nuclei, rXH (0.102 nm) and the CSA of X.  dt in time_unit, D in 1 / time_unit,
    field_MHz the proton frequency.  Returns dict(R1, R2, NOE (nV each, R1 and R2 in 1/s), J (nV, 5) in time_unit, omega (5)).  No
    error estimate (the module's docstring)."""
    from .spectral_densities import relaxationModel
    R = relaxationModel(nuclei, 2.0 * np.pi * float(field_MHz) * 1.0e6 / 267.513e6)
    R.set_time_unit(time_unit)
    if rXH is not None:
        R.rXH = float(rXH)
    Jw = J(result, D, R.omega, dt, stop=stop)
    fDD, fCSA, tf, gr = R.get_f_DD(), R.get_f_CSA(csa), R.time_fact, R.gH.gamma / R.gX.gamma
    J0, J1, J2, J3, J4 = (Jw[:, k] for k in range(5))
    R1 = tf * (fDD * (J2 + 3 * J1 + 6 * J4)) + fCSA * (tf * J1)
    R2 = tf * (0.5 * fDD * (4 * J0 + J2 + 3 * J1 + 6 * J4 + 6 * J3)) + fCSA * (tf * (1.0 / 6.0 * (4 * J0 + 3 * J1)))
    NOE = 1.0 + tf * gr / R1 * fDD * (6 * J4 - J2)
    return dict(R1=R1, R2=R2, NOE=NOE, J=Jw, omega=R.omega.copy())
