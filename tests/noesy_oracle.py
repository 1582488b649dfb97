"""
CPU definitions for the NOESY tests (tests/test_noesy_host.py, tests/test_gpu_noesy.py): plain numpy / scipy, nothing of the package
beyond the pair order of noe.pair_index, which is written out here.

    J(w)     = S2 tc / (1 + w^2 tc^2) + (1 - S2) t' / (1 + w^2 t'^2),      1 / t' = 1 / tc + 1 / te
    sigma_ij = q A6 [6 J(2w) - J(0)],       rho_ij = q A6 [J(0) + 3 J(w) + 6 J(2w)]
    R_ij = sigma_ij,  R_ii = sum_j rho_ij + leak_i,       A(tau) = exp(-R tau)
"""
import functools

import numpy as np

GAMMA_H = 267.513e6
Q_HH = 0.10 * 1.1121216813552401e-82 * GAMMA_H ** 4.0        # 0.1 (mu0 / 4 pi)^2 hbar^2 gamma_H^4, SI
U53 = 2.0 ** -53


def omega_H(field_MHz):
    return 2.0 * np.pi * field_MHz * 1e6


def pairs(P):
    """(npairs, 2): row-major over i < j"""
    i, j = np.triu_indices(P, 1)
    return np.stack([i, j], axis=1)


def J(w, S2, tc, te):
    tp = tc * te / (tc + te)
    return S2 * tc / (1.0 + w * w * tc * tc) + (1.0 - S2) * tp / (1.0 + w * w * tp * tp)


def pair_rates(A6, S2, w, tc, te, q):
    """sigma, rho and the sum of magnitudes q A6 (J(0) + 6 J(2w)) that bounds sigma's rounding, per pair"""
    S2 = np.clip(S2, 0.0, 1.0)
    J0, J1, J2 = J(0.0, S2, tc, te), J(w, S2, tc, te), J(2.0 * w, S2, tc, te)
    return q * A6 * (6.0 * J2 - J0), q * A6 * (J0 + 3.0 * J1 + 6.0 * J2), q * A6 * (J0 + 6.0 * J2)


def rate_matrix(A6, S2, P, w, tc, te, leak, q):
    """R (P, P), the per-pair rho as a symmetric (P, P) matrix with zero diagonal, and sigma's magnitude sum likewise"""
    sig, rho, mag = pair_rates(A6, S2, w, tc, te, q)
    pr = pairs(P)

    def full(v):
        M = np.zeros((P, P))
        M[pr[:, 0], pr[:, 1]] = v
        M[pr[:, 1], pr[:, 0]] = v
        return M
    R, RHO, MAG = full(sig), full(rho), full(mag)
    R[np.arange(P), np.arange(P)] = RHO.sum(axis=1) + leak
    return R, RHO, MAG


def expm_scipy(R, tau):
    from scipy.linalg import expm
    return expm(-R * tau)


def expm_eigh(R, tau):
    lam, V = np.linalg.eigh(R)
    return (V * np.exp(-lam * tau)) @ V.T


@functools.lru_cache(maxsize=None)
def synthetic(P, seed=0):
    """The synthetic rate input: P points uniform in a cube at 0.06 protons / A^3, distances clamped to >= 1.6 A, S2 uniform in
    [0.3, 0.95]: (A6 in A^-6, S2), per pair, read-only"""
    rng = np.random.default_rng(1000 * P + seed)
    side = (P / 0.06) ** (1.0 / 3.0)
    x = rng.uniform(0.0, side, (P, 3))
    pr = pairs(P)
    r = np.maximum(np.linalg.norm(x[pr[:, 0]] - x[pr[:, 1]], axis=1), 1.6)
    A6 = r ** -6.0
    S2 = rng.uniform(0.3, 0.95, pr.shape[0])
    for a in (A6, S2, r):
        a.setflags(write=False)
    return A6, S2, r


Q_ANGSTROM = Q_HH * 1e-10 ** -6.0           # the prefactor for coordinates in Angstrom
Q_NM = Q_HH * 1e-9 ** -6.0
FIELD = 600.0
LEAK = 0.5
TAU_C = (5e-9, 0.3e-9)
TAU_E = 5e-11


@functools.lru_cache(maxsize=None)
def synthetic_R(P, tc, seed=0):
    """R of the synthetic input at 600 MHz, leak 0.5 / s, tau_e = 50 ps (read-only)"""
    A6, S2, _ = synthetic(P, seed)
    R = rate_matrix(A6, S2, P, omega_H(FIELD), tc, TAU_E, LEAK, Q_ANGSTROM)[0]
    R.setflags(write=False)
    return R
