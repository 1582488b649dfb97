"""
The index algebra of the blocked Wiener-Khinchin C(t) (spinrelax_amd/csrc/sr_ct_long.hip), restated in numpy float64 and held
against the oracle's calculate_Ct_Palmer on a machine without a GPU: mean-removed signals of the traceless decomposition,
block spectra of zero-padded blocks, cross-spectra per block offset, the two-piece recombination -- written out
(c_d[m] + c_{d+1}[B + m]) and in the fused form the kernels use (Q_d = P_d + (-1)^k P_{d+1}, one inverse per offset) -- and
the float64 restoration of what the mean subtraction removed, including odd F and a zero-filled last block.
"""
import numpy as np
import pytest

import sr_oracle as o
from spinrelax_amd import synth

W6 = (1.0, 3.0, 12.0, 12.0, 12.0, 2.0)           # 6 x the weights 1/6, 1/2, 2, 2, 2 (traceless components) and 1/3 (trace)


def signals(u):
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    return [2 * z * z - x * x - y * y, x * x - y * y, x * y, x * z, y * z, x * x + y * y + z * z]


def blocked_lag_sums(u, B, fused, unit):
    """S[D] = sum_j (u_j . u_{j+D})^2, D = 0 .. F // 2, of one series u (F, 3) by the blocked form with blocks of B samples."""
    F = u.shape[0]
    L = F // 2
    M = 2 * B
    nb = -(-F // B)
    nd = L // B + 1
    a = signals(u)
    nsig = 5 if unit else 6
    # any constant m_c gives an exact identity: the chunk mean, coarsely rounded as the kernel's is
    m = [np.round(np.mean(a[c]), 3) for c in range(nsig)]
    e = np.zeros(F)
    K = 0.0
    P = np.zeros((nd + 2, B + 1), dtype=np.complex128)
    for c in range(nsig):
        d = a[c] - m[c]
        e += W6[c] * m[c] * d
        K += W6[c] * m[c] ** 2
        pad = np.zeros(nb * B)
        pad[:F] = d                                        # the last block is zero-filled
        X = np.fft.rfft(pad.reshape(nb, B), n=M, axis=1)   # (nb, B + 1)
        for off in range(min(nd + 1, nb)):
            P[off] += W6[c] * np.sum(np.conj(X[:nb - off]) * X[off:], axis=0)
    if unit:                                               # |u|^2 |u'|^2 / 3 with |u|^2 = 1 + eps: eps / 3 joins e, 1/3 joins K
        e += 2.0 * (a[5] - 1.0)
        K += 2.0
    PE = np.concatenate([[0.0], np.cumsum(e)])
    S = np.empty(L + 1)
    sign = (-1.0) ** np.arange(B + 1)
    cd = [np.fft.irfft(P[off], n=M) for off in range(nd + 1)]
    for off in range(nd):
        q = np.fft.irfft(P[off] + sign * P[off + 1], n=M)[:B] if fused else None
        for mm in range(B):
            D = off * B + mm
            if D > L:
                break
            piece = q[mm] if fused else cd[off][mm] + (cd[off + 1][B + mm] if mm > 0 else 0.0)
            S[D] = (piece + PE[F - D] + PE[F] - PE[D] + (F - D) * K) / 6.0
    return S


def blocked_ct(v4, B, fused, unit=True):
    R, F, V, _ = v4.shape
    L = F // 2
    p = np.empty((R, L, V))
    for r in range(R):
        for v in range(V):
            S = blocked_lag_sums(v4[r, :, v].astype(np.float64), B, fused, unit)
            p[r, :, v] = 1.5 * S[1:] / (F - np.arange(1, L + 1)) - 0.5
    Ct = p.mean(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        dCt = p.std(axis=0) / (np.sqrt(R) - 1.0)
    return Ct, dCt


def relerr(a, b):
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))


@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('F,B', [(8193, 4096), (12288, 4096), (13001, 4096), (100, 16), (101, 16), (96, 32), (33, 8), (1000, 64)])
def test_blocked_form_equals_direct_sums(F, B, fused):
    R, V = 2, 1
    v4 = synth.synth_vectors(R * F, V, seed=F).reshape(R, F, V, 3)
    Cr, dCr = o.calculate_Ct_Palmer(v4)
    Ct, dCt = blocked_ct(v4, B, fused)
    assert relerr(Ct, Cr) < 1e-12, (F, B, relerr(Ct, Cr))
    assert np.max(np.abs(dCt - dCr)) < 1e-12


@pytest.mark.parametrize('F,B', [(101, 16), (1000, 64)])
def test_blocked_form_series_that_are_not_unit_vectors(F, B):
    """the sixth signal |u|^2 instead of the eps term"""
    R, V = 2, 2
    v = synth.synth_vectors(R * F, V, seed=3).copy()
    v[:, 0] *= np.float32(1.7)
    v[10:20, 1] = 0.0
    v4 = v.reshape(R, F, V, 3)
    Cr, dCr = o.calculate_Ct_Palmer(v4)
    Ct, dCt = blocked_ct(v4, B, True, unit=False)
    assert relerr(Ct, Cr) < 1e-12 and np.max(np.abs(dCt - dCr)) < 1e-12
