"""
CPU tests (no GPU) of the blocked form of the pair cross-correlation functions (spinrelax_amd/csrc/sr_ct_cross_long.hip):
  * its index algebra in numpy float64 on TWO series -- block spectra of zero-padded blocks, cross-spectra conj(X^i_a) X^j_{a+d} per
    block offset, the recombination S_ij[d B + m] = c_d[m] + c_{d+1}[B + m] written out and in the fused form the kernels use
    (Q_d = P_d + (-1)^k P_{d+1}, one inverse per offset) -- for both directions and their mean, against the lag-by-lag definition;
  * the float64 restoration of what the subtraction of the chunk constants removed (one suffix sum of h[t'] = e_ij[F-1-t'] + e_ji[t']
    and (F - k) K_ij), with a series that is not a unit-vector series and with i = j;
  * the FFT oracle that tests/test_gpu_ct_cross_long.py holds the kernels against, itself against the definition;
  * the new entry points in the header, the binding and the library, and the help text of --crossCt.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from spinrelax_amd import _lib

SCRIPT = os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')
NEW = {'sr_ct_cross_long_max_frames': 1, 'sr_ct_cross_long_f32_dev': 17, 'sr_vectors_ct_cross_long_f32': 13,
       'sr_vectors_ct_cross_long_err_f32': 14}
W6 = (1.0, 3.0, 12.0, 12.0, 12.0, 2.0)           # 6 x the weights 1/6, 1/2, 2, 2, 2 (traceless components) and 1/3 (trace)


# ---- vectors and oracles shared with tests/test_gpu_ct_cross_long.py ------------------------------------------------------------------
def make_vectors(N, seed, nV):
    """unit vectors (N, nV, 3) float32 as make_vectors of tests/test_gpu_ct_cross.py: an AR(1) wobble of about 0.15 rad around axes within
    15 degrees of z; the recursion x_t = 0.95 x_{t-1} + n_t runs in blocks of 256 frames (a triangular matrix of powers per block)"""
    rng = np.random.default_rng(seed)
    tilt, az = np.radians(15.0) * rng.random(nV), 2 * np.pi * rng.random(nV)
    axis = np.stack((np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)), axis=-1)
    e1 = np.cross(axis, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1, axis=-1, keepdims=True)
    e2 = np.cross(axis, e1)
    noise = 0.15 * np.sqrt(1 - 0.95 ** 2) * rng.standard_normal((N, nV * 2))
    x = 0.15 * rng.standard_normal(nV * 2)
    blk = 256
    idx = np.arange(blk)
    T = np.tril(0.95 ** np.maximum(idx[:, None] - idx[None, :], 0))          # T[t, s] = 0.95^(t - s), s <= t
    decay = 0.95 ** (idx + 1)
    w = np.empty((N, nV * 2))
    for b in range(0, N, blk):
        n = min(blk, N - b)
        w[b:b + n] = T[:n, :n] @ noise[b:b + n] + decay[:n, None] * x[None]
        x = w[b + n - 1]
    w = w.reshape(N, nV, 2)
    u = axis[None] + w[..., :1] * e1[None] + w[..., 1:] * e2[None]
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    u = u.astype(np.float32)
    return u / np.linalg.norm(u, axis=-1, keepdims=True).astype(np.float32)


def oracle_cross(v4, pairs, sym, lags=None):
    """tests/test_gpu_ct_cross.py::oracle_cross, the definition lag by lag in float64: v4 (R, F, V, 3) -> P0 (nP), C and dC (L, nP)"""
    v4 = np.asarray(v4, dtype=np.float64)
    R, F = v4.shape[:2]
    L = F // 2
    ks = np.arange(0, L + 1) if lags is None else np.concatenate(([0], np.asarray(lags)))
    P = np.empty((len(ks), R, len(pairs)))
    for n, (i, j) in enumerate(pairs):
        a, b = v4[:, :, i], v4[:, :, j]
        for m, k in enumerate(ks):
            S = (np.einsum('rtc,rtc->rt', a[:, :F - k], b[:, k:]) ** 2).sum(axis=1)
            if sym:
                S = 0.5 * (S + (np.einsum('rtc,rtc->rt', b[:, :F - k], a[:, k:]) ** 2).sum(axis=1))
            P[m, :, n] = 1.5 * S / (F - k) - 0.5
    with np.errstate(divide='ignore', invalid='ignore'):
        dC = np.std(P[1:], axis=1) / (np.sqrt(R) - 1.0)
    return P[0].mean(axis=0), P[1:].mean(axis=1), dC


def oracle_cross_fft(v4, pairs, sym):
    """The same numbers for long chunks: (u_i . u_j)^2 = sum over the six products xx, yy, zz, 2 xy, 2 xz, 2 yz of u_i times the same
    product of u_j, so S_ij is the sum of six cross-correlations, each one zero-padded float64 numpy.fft transform pair"""
    v4 = np.asarray(v4, dtype=np.float64)
    R, F = v4.shape[:2]
    L = F // 2
    n = 1 << int(np.ceil(np.log2(F + L + 1)))
    x, y, z = v4[..., 0], v4[..., 1], v4[..., 2]                               # (R, F, V)
    prod = np.stack((x * x, y * y, z * z, x * y, x * z, y * z), axis=0)        # (6, R, F, V)
    g = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])[:, None, None]
    vs = sorted(set(int(v) for v in np.asarray(pairs).ravel()))
    spec = {v: np.fft.rfft(prod[..., v], n=n, axis=2) for v in vs}             # (6, R, n/2 + 1)
    P = np.empty((L + 1, R, len(pairs)))
    norm = F - np.arange(L + 1)
    for m, (i, j) in enumerate(pairs):
        S = np.fft.irfft((g * np.conj(spec[int(i)]) * spec[int(j)]).sum(axis=0), n=n, axis=1)[:, :L + 1]
        if sym:
            S = 0.5 * (S + np.fft.irfft((g * np.conj(spec[int(j)]) * spec[int(i)]).sum(axis=0), n=n, axis=1)[:, :L + 1])
        P[:, :, m] = (1.5 * S / norm - 0.5).T
    with np.errstate(divide='ignore', invalid='ignore'):
        dC = np.std(P[1:], axis=1) / (np.sqrt(R) - 1.0)
    return P[0].mean(axis=0), P[1:].mean(axis=1), dC


# ---- the blocked form on two series, numpy float64 ---------------------------------------------------------------------------------------
def signals(u):
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    return [2 * z * z - x * x - y * y, x * x - y * y, x * y, x * z, y * z, x * x + y * y + z * z]


def definition(ui, uj):
    """S_ij[k] = sum_t (u_i(t) . u_j(t + k))^2, k = 0 .. F // 2: the later frame from j"""
    F = ui.shape[0]
    return np.array([np.sum(np.einsum('tc,tc->t', ui[:F - k], uj[k:]) ** 2) for k in range(F // 2 + 1)])


def blocked_pair_sums(ui, uj, B, fused, six, means=True):
    """S_ij[D], D = 0 .. F // 2, of two series (F, 3) by the blocked form with blocks of B samples.  six: |u|^2 as a sixth signal of both
    series (needed unless both are unit-vector series); means: subtract a constant per (series, signal) before the transforms and
    restore what that removed, as the kernels do -- False: the bare identity on the signals themselves."""
    F = ui.shape[0]
    L = F // 2
    M = 2 * B
    nb = -(-F // B)
    nd = L // B + 1
    ai, aj = signals(ui), signals(uj)
    nsig = 6 if six else 5
    # any constants give an exact identity: the chunk means, coarsely rounded as the kernel's are, each series its own
    mi = [np.round(np.mean(ai[c]), 3) if means else 0.0 for c in range(nsig)]
    mj = [np.round(np.mean(aj[c]), 3) if means else 0.0 for c in range(nsig)]
    eij, eji = np.zeros(F), np.zeros(F)
    K = 0.0
    P = np.zeros((nd + 2, B + 1), dtype=np.complex128)
    for c in range(nsig):
        di, dj = ai[c] - mi[c], aj[c] - mj[c]
        eij += W6[c] * mj[c] * di
        eji += W6[c] * mi[c] * dj
        K += W6[c] * mi[c] * mj[c]
        pi, pj = np.zeros(nb * B), np.zeros(nb * B)
        pi[:F], pj[:F] = di, dj                                  # the last block is zero-filled
        Xi = np.fft.rfft(pi.reshape(nb, B), n=M, axis=1)         # (nb, B + 1)
        Xj = np.fft.rfft(pj.reshape(nb, B), n=M, axis=1)
        for off in range(min(nd + 1, nb)):
            P[off] += W6[c] * np.sum(np.conj(Xi[:nb - off]) * Xj[off:], axis=0)
    if not six:                                                  # |u_i|^2 |u_j|^2 / 3 with |u|^2 = 1 + eps: eps / 3 joins e, 1/3 joins K
        eij += 2.0 * (ai[5] - 1.0)
        eji += 2.0 * (aj[5] - 1.0)
        K += 2.0
    # sum_{t < F-D} e_ij[t] + sum_{t >= D} e_ji[t] as ONE suffix sum over t' >= D of h[t'] = e_ij[F - 1 - t'] + e_ji[t']
    h = eij[::-1] + eji
    suffix = np.concatenate((np.cumsum(h[::-1])[::-1], [0.0]))
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
            S[D] = (piece + suffix[D] + (F - D) * K) / 6.0
    return S


def series(F, seed, nV=2):
    return make_vectors(F, seed, nV).astype(np.float64)


@pytest.mark.parametrize('fused', [False, True])
def test_two_series_blocked_identity(fused):
    """B = 16, every F in 17 .. 70, L = F // 2: nb = 2 .. 5, a last block of one sample (F = 17, 33, 49, 65), L a multiple of B (F = 32,
    33, 64, 65); both directions and their mean against the definition"""
    B = 16
    for F in range(17, 71):
        u = series(F, seed=F)
        ui, uj = u[:, 0], u[:, 1]
        Sij, Sji = blocked_pair_sums(ui, uj, B, fused, True, means=False), blocked_pair_sums(uj, ui, B, fused, True, means=False)
        Dij, Dji = definition(ui, uj), definition(uj, ui)
        assert np.max(np.abs(Sij - Dij) / Dij) < 1e-12, F
        assert np.max(np.abs(Sji - Dji) / Dji) < 1e-12, F
        assert np.max(np.abs(Dij[1:] - Dji[1:])) > 1e-3                   # the two directions are different functions
        assert np.max(np.abs(0.5 * (Sij + Sji) - 0.5 * (Dij + Dji)) / (0.5 * (Dij + Dji))) < 1e-12, F


@pytest.mark.parametrize('F,B', [(17, 16), (64, 16), (65, 16), (70, 16), (1000, 64), (8193, 4096)])
def test_mean_restoration(F, B):
    """transform of the deviations + suffix sum + (F - k) K_ij = the definition, to 1e-12: unit pairs by the eps term, a pair with a
    series that is not a unit-vector series by the sixth signal of both, and i = j"""
    u = series(F, seed=3 * F + 1, nV=3)
    u[:, 2] *= 1.7                                                        # not a unit-vector series
    u[F // 3:F // 3 + 3, 2] = 0.0
    for i, j, six in ((0, 1, False), (1, 0, False), (0, 0, False), (0, 2, True), (2, 1, True), (2, 2, True), (0, 1, True)):
        S = blocked_pair_sums(u[:, i], u[:, j], B, True, six)
        D = definition(u[:, i], u[:, j])
        # a unit pair drops eps_i eps_j / 3 per frame, eps below 1.2e-7 for float32 unit vectors: 5e-15 relative
        assert np.max(np.abs(S - D) / D) < 1e-12, (F, i, j, six)


def test_fft_oracle_against_the_definition():
    F, R, V = 300, 3, 4
    v4 = make_vectors(R * F, seed=11, nV=V).reshape(R, F, V, 3).copy()
    v4[:, :, 3] *= np.float32(1.7)
    pairs = np.array([(0, 0), (1, 2), (2, 1), (3, 1), (1, 2)], dtype=np.int32)
    for sym in (0, 1):
        a, b = oracle_cross_fft(v4, pairs, sym), oracle_cross(v4, pairs, sym)
        for x, y in zip(a, b):
            assert x.shape == y.shape and np.max(np.abs(x - y)) < 1e-12


def test_make_vectors_keeps_every_C_above_the_bar_of_a_relative_error():
    v4 = make_vectors(2 * 700, seed=5, nV=4).reshape(2, 700, 4, 3)
    assert np.max(np.abs(np.linalg.norm(v4.astype(np.float64), axis=-1) - 1.0)) < 2e-7
    _, C, _ = oracle_cross_fft(v4, [(0, 0), (1, 2), (3, 1)], 1)
    assert np.min(C) > 0.4


def test_abi_declares_the_new_entry_points():
    with open(os.path.join(ROOT, 'include', 'spinrelax_hip.h')) as fp:
        text = re.sub(r'/\*.*?\*/', '', fp.read(), flags=re.S)
    for name, nargs in NEW.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        m = re.search(r'\b(int|int64_t) %s\((.*?)\);' % name, text, flags=re.S)
        assert m and len(m.group(2).split(',')) == nargs, name
        # the blocked counterpart takes the arguments of the function it stands beside
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace('_long', '')]
    assert _lib.SIGNATURES['sr_ct_cross_long_max_frames'][0] is ctypes.c_int64
    assert 'SR_ABI_VERSION 13' in open(os.path.join(ROOT, 'include', 'spinrelax_hip.h')).read() and _lib.ABI_VERSION == 13


def test_library_exports_the_new_entry_points():
    if not os.path.isfile(_lib.LIB_PATH):
        from spinrelax_amd import build
        build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    assert lib.sr_ct_cross_long_max_frames(None) == -1                    # no context: refused on the host, nothing touched


def test_help_states_no_short_limit_for_crossCt():
    p = subprocess.run([sys.executable, SCRIPT, '--help'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0
    text = ' '.join(p.stdout.decode().split())
    for flag in ('--crossCt', '--pairs', '--asym', '--tau', '--Ct'):
        assert flag in text
    assert '--vecRot has no effect' in text
    assert '6624' not in text
    assert 'Any --tau that --Ct accepts' in text
    with open(SCRIPT) as fp:
        assert '6624' not in fp.read()
