"""
numpy float64 oracles of the fully anisotropic (rhombic) rotational-diffusion model, for the tests of model 3 of
sr_jomega_relax_f64 and of the host helpers (a plain helper module; the reference has no working form of this model).

Two independent forms of J(omega) of C(t) = S2 + sum_k C_k exp(-t/tau_k) for a unit vector v in the principal-axis frame of
the tensor (Dx, Dy, Dz):

  closed form    Woessner 1962 / Ghose, Fushman & Cowburn 2001: five rates d_j and five amplitudes A_j(v) written out.
  operator form  H = Dx Lx^2 + Dy Ly^2 + Dz Lz^2 in the 5 x 5 l = 2 angular-momentum matrices, q = sqrt(4 pi / 5) Y_2m(v),
                 J(omega) = Re q^+ (H + k) ((H + k)^2 + omega^2)^-1 q, evaluated through numpy's eigendecomposition of H: it
                 knows neither the d_j nor the A_j.

and, on top of either, the table sr_jomega_relax_f64 returns (R1, R2, NOE, rho, J and the 12 rsCSA statistics as weighted
mean / sigma over a vector distribution), with numpy.average and a second pass about the mean.
"""
import numpy as np


# ---- closed form -----------------------------------------------------------------------------------------------------------
def rates_closed(D):
    Dx, Dy, Dz = D
    Diso = (Dx + Dy + Dz) / 3.0
    L2 = (Dx * Dy + Dx * Dz + Dy * Dz) / 3.0
    R = np.sqrt(max(Diso * Diso - L2, 0.0))
    return np.array([4 * Dx + Dy + Dz, Dx + 4 * Dy + Dz, Dx + Dy + 4 * Dz, 6 * Diso + 6 * R, 6 * Diso - 6 * R]), Diso, R


def amplitudes_closed(v, D):
    v = np.asarray(v, dtype=float)
    _, Diso, R = rates_closed(D)
    delta = np.zeros(3) if R == 0 else (np.asarray(D, dtype=float) - Diso) / R
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    dd = 0.25 * (3.0 * (x ** 4 + y ** 4 + z ** 4) - 1.0)
    e = (delta[0] * (3 * x ** 4 + 6 * y ** 2 * z ** 2 - 1) + delta[1] * (3 * y ** 4 + 6 * x ** 2 * z ** 2 - 1)
         + delta[2] * (3 * z ** 4 + 6 * x ** 2 * y ** 2 - 1)) / 12.0
    return np.stack((3 * y ** 2 * z ** 2, 3 * x ** 2 * z ** 2, 3 * x ** 2 * y ** 2, dd - e, dd + e), axis=-1)


def _g(x, y):
    return x / (x * x + y * y)


def J_closed(om, v, D, S2, C, tau):
    """(..., len(om))"""
    om = np.atleast_1d(np.asarray(om, dtype=float))
    d = rates_closed(D)[0][:, None]
    G = S2 * _g(d, om)
    for c, t in zip(C, tau):
        G = G + c * _g(d + 1.0 / t, om)
    return amplitudes_closed(v, D) @ G


# ---- operator form ---------------------------------------------------------------------------------------------------------
def _l2_matrices():
    m = np.arange(2, -3, -1)                       # basis |2, m>, m = 2 .. -2
    Lz = np.diag(m).astype(complex)
    Lp = np.zeros((5, 5), dtype=complex)           # L+ |m> = sqrt(l(l+1) - m(m+1)) |m+1>
    for i, mm in enumerate(m):
        if mm < 2:
            Lp[i - 1, i] = np.sqrt(6.0 - mm * (mm + 1))
    Lm = Lp.conj().T
    return (Lp + Lm) / 2.0, (Lp - Lm) / 2.0j, Lz


def _q(v):
    """sqrt(4 pi / 5) Y_2m(v), m = 2 .. -2: (..., 5)"""
    v = np.asarray(v, dtype=float)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    xp, xm = x + 1j * y, x - 1j * y
    return np.stack((np.sqrt(3.0 / 8.0) * xp * xp, -np.sqrt(1.5) * z * xp, 0.5 * (3 * z * z - 1) + 0j,
                     np.sqrt(1.5) * z * xm, np.sqrt(3.0 / 8.0) * xm * xm), axis=-1)


def J_operator(om, v, D, S2, C, tau):
    """(..., len(om))"""
    om = np.atleast_1d(np.asarray(om, dtype=float))
    Lx, Ly, Lz = _l2_matrices()
    H = D[0] * Lx @ Lx + D[1] * Ly @ Ly + D[2] * Lz @ Lz
    ev, U = np.linalg.eigh(H)
    p = np.abs(_q(v) .conj() @ U) ** 2             # (..., 5) weight of every eigenvector in q
    G = S2 * _g(ev[:, None], om)
    for c, t in zip(C, tau):
        G = G + c * _g(ev[:, None] + 1.0 / t, om)
    return p @ G


# ---- the table of sr_jomega_relax_f64 --------------------------------------------------------------------------------------
def _quantities(J, fDD, fCSA, tf, gr):
    """J (..., 5) -> (..., 14): R1, R2, NOE (per-vector R1), rho, N, J0..J4, a1, b1, a2, b2"""
    J0, J1, J2, J3, J4 = (J[..., k] for k in range(5))
    a1 = tf * (fDD * (J2 + 3 * J1 + 6 * J4))
    b1 = tf * J1
    a2 = tf * (0.5 * fDD * (4 * J0 + J2 + 3 * J1 + 6 * J4 + 6 * J3))
    b2 = tf * (1.0 / 6.0 * (4 * J0 + 3 * J1))
    R1 = a1 + fCSA * b1
    R2 = a2 + fCSA * b2
    N = 6 * J4 - J2
    return np.stack((R1, R2, 1.0 + tf * gr / R1 * fDD * N, J1 / J0, N, J0, J1, J2, J3, J4, a1, b1, a2, b2), axis=-1)


def relax_table(D, omega, fDD, fCSA, tf, gr, S2, C, tau, K, vecs, weights=None, per_residue=False, noe_mode=0, form='operator'):
    """The outputs of model 3: out (E, n, 4, 2), J (E, n, 5, 2), stats (E, n, 12).
    vecs (B, 3) shared by every residue with weights (n, B) or None; per_residue: vecs (n, 3), sigma 0."""
    Jfun = J_operator if form == 'operator' else J_closed
    omega = np.atleast_2d(omega)
    E, n = omega.shape[0], len(S2)
    fDD, tf, gr = (np.broadcast_to(a, (E,)) for a in (fDD, tf, gr))
    fCSA = np.broadcast_to(fCSA, (E, n))
    out, Jo, st = np.zeros((E, n, 4, 2)), np.zeros((E, n, 5, 2)), np.zeros((E, n, 12))
    for e in range(E):
        for i in range(n):
            k = int(K[i])
            v = vecs[i] if per_residue else vecs
            q = _quantities(Jfun(omega[e], v, D, S2[i], C[i, :k], tau[i, :k]), fDD[e], fCSA[e, i], tf[e], gr[e])
            if per_residue:
                mean, var, c1, c2 = q, np.zeros(14), 0.0, 0.0
            else:
                w = None if weights is None else weights[i]
                mean = np.average(q, axis=0, weights=w)
                var = np.average((q - mean) ** 2, axis=0, weights=w)
                c1 = np.average((q[:, 10] - mean[10]) * (q[:, 11] - mean[11]), weights=w)
                c2 = np.average((q[:, 12] - mean[12]) * (q[:, 13] - mean[13]), weights=w)
            sig = np.sqrt(var)
            out[e, i, 0], out[e, i, 1], out[e, i, 3] = (mean[0], sig[0]), (mean[1], sig[1]), (mean[3], sig[3])
            if noe_mode == 0:
                out[e, i, 2] = mean[2], sig[2]
            else:
                c = tf[e] * gr[e] / mean[0] * fDD[e]
                out[e, i, 2] = 1.0 + c * mean[4], abs(c) * sig[4]
            Jo[e, i, :, 0], Jo[e, i, :, 1] = mean[5:10], sig[5:10]
            st[e, i] = [mean[10], mean[11], var[10], c1, var[11], mean[12], mean[13], var[12], c2, var[13], mean[4], var[4]]
    return out, Jo, st
