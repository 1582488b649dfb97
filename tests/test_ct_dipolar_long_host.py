"""
CPU tests (no GPU) of the blocked forms of the two distance-weighted correlation functions (spinrelax_amd/csrc/sr_ct_dipolar_long.hip):
  * the FFT oracles that tests/test_gpu_ct_dipolar_long.py holds the kernels against -- the definition as zero-padded float64 numpy.fft
    correlations of the six products of a (x) a and of w, chunk-pooled like the library -- themselves against the lag-by-lag oracles of
    tests/test_gpu_ct_dipolar.py and tests/test_gpu_ct_dipolar_cross.py: 1e-12;
  * the identity the kernels rest on: with |a|^2 = w, 1.5 (a . a')^2 - 0.5 w w' = 1.5 Q : Q', Q the traceless part of a (x) a.  On planes
    rounded to float32 |a|^2 and w differ by the rounding: five signals in float64 against the definition on the same planes at
    F = 10017, bar 1e-7 relative (1.5e-9 measured), a factor of ten below the 1e-6 the GPU tests hold the kernels to;
  * the new entry points in the header, the binding and the library;
  * the dispatch of spinrelax_amd.ct on a stub of the resident vectors.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, relerr
from test_gpu_ct_dipolar import make_pairs, oracle_dipolar, planes_of
from test_gpu_ct_dipolar_cross import oracle_dcross
from spinrelax_amd import _lib
from spinrelax_amd import ct as hostct

NEW = {'sr_ct_dipolar_long_max_frames': 1, 'sr_ct_dipolar_cross_long_max_frames': 1, 'sr_ct_dipolar_long_f32_dev': 12,
       'sr_vectors_ct_dipolar_long_f32': 12, 'sr_ct_dipolar_cross_long_f32_dev': 18, 'sr_vectors_ct_dipolar_cross_long_f32': 16}
G6 = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])[:, None, None, None]


# ---- the FFT oracles, shared with tests/test_gpu_ct_dipolar_long.py -----------------------------------------------------------------------
def products(a4):
    """the six products xx, yy, zz, xy, xz, yz of a4 (R, F, V, 3): (6, R, F, V); (a . a')^2 is their G6-weighted sum of products"""
    x, y, z = a4[..., 0], a4[..., 1], a4[..., 2]
    return np.stack((x * x, y * y, z * z, x * y, x * z, y * z), axis=0)


def lag_sums(A, B, L):
    """sum_t A[.., t, v] B[.., t + k, v], k = 0 .. L, along the frame axis (-2), by zero-padded float64 transforms"""
    F = A.shape[-2]
    n = 1 << int(np.ceil(np.log2(F + L + 1)))
    S = np.fft.irfft(np.conj(np.fft.rfft(A, n=n, axis=-2)) * np.fft.rfft(B, n=n, axis=-2), n=n, axis=-2)
    return S[..., :L + 1, :]


def fft_core(a4, w4):
    """a4 (R, F, V, 3), w4 (R, F, V) -> C, dC (L, V), <w>, <w^2> (V): oracle_core of tests/test_gpu_ct_dipolar.py by transforms"""
    a4, w4 = np.asarray(a4, dtype=np.float64), np.asarray(w4, dtype=np.float64)
    R, F = w4.shape[:2]
    L = F // 2
    p = products(a4)
    Sa = (G6 * lag_sums(p, p, L)).sum(axis=0)                                  # (R, L + 1, V)
    Sw = lag_sums(w4, w4, L)
    c = ((1.5 * Sa - 0.5 * Sw) / (F - np.arange(L + 1))[None, :, None])[:, 1:]
    n = ((w4 ** 2).sum(axis=1) / F).mean(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        dC = np.std(c, axis=0) / (np.sqrt(R) - 1.0) / n
    return c.mean(axis=0) / n, dC, w4.mean(axis=(0, 1)), (w4 ** 2).mean(axis=(0, 1))


def fft_cross_core(a4, w4, pairs, sym):
    """-> P0, dP0 (nP), C, dC (L, nP), <w^2> (V): oracle_core of tests/test_gpu_ct_dipolar_cross.py by transforms"""
    a4, w4 = np.asarray(a4, dtype=np.float64), np.asarray(w4, dtype=np.float64)
    pairs = np.asarray(pairs)
    R, F = w4.shape[:2]
    L = F // 2
    p = products(a4)
    pi, pj, wi, wj = p[..., pairs[:, 0]], p[..., pairs[:, 1]], w4[..., pairs[:, 0]], w4[..., pairs[:, 1]]
    Sa = (G6 * lag_sums(pi, pj, L)).sum(axis=0)
    Sw = lag_sums(wi, wj, L)
    if sym:
        Sa = 0.5 * (Sa + (G6 * lag_sums(pj, pi, L)).sum(axis=0))
        Sw = 0.5 * (Sw + lag_sums(wj, wi, L))
    c = (1.5 * Sa - 0.5 * Sw) / (F - np.arange(L + 1))[None, :, None]          # (R, L + 1, nP)
    n = ((w4 ** 2).sum(axis=1) / F).mean(axis=0)
    norm = np.sqrt(n[pairs[:, 0]] * n[pairs[:, 1]])
    with np.errstate(divide='ignore', invalid='ignore'):
        d = np.std(c, axis=0) / (np.sqrt(R) - 1.0) / norm
    m = c.mean(axis=0) / norm
    return m[0], d[0], m[1:], d[1:], (w4 ** 2).mean(axis=(0, 1))


def chunks(a, w, R, F, starts):
    starts = np.arange(R) * F if starts is None else starts
    return np.stack([a[s:s + F] for s in starts]), np.stack([w[s:s + F] for s in starts])


def oracle_dipolar_fft(vec, dist, R, F, starts=None):
    """oracle_dipolar of tests/test_gpu_ct_dipolar.py for long chunks: C, dC, reff6, reff3, S2rad"""
    a, w, rref = planes_of(vec, dist)
    C, dC, w1, w2 = fft_core(*chunks(a, w, R, F, starts))
    return C, dC, rref * w2 ** (-1.0 / 6.0), rref * w1 ** (-1.0 / 3.0), w1 * w1 / w2


def oracle_dcross_fft(vec, dist, pairs, sym, R, F, starts=None):
    """oracle_dcross of tests/test_gpu_ct_dipolar_cross.py for long chunks: P0, dP0, C, dC, reff6 (nP, 2)"""
    a, w, rref = planes_of(vec, dist)
    P0, dP0, C, dC, w2 = fft_cross_core(*chunks(a, w, R, F, starts), pairs, sym)
    return P0, dP0, C, dC, (rref * w2 ** (-1.0 / 6.0))[np.asarray(pairs)]


def test_fft_oracles_against_the_lag_by_lag_oracles():
    F, R, V = 300, 3, 4
    u, r, raw = make_pairs(R * F + 40, seed=21, nV=V)
    pairs = np.array([(0, 0), (1, 2), (2, 1), (3, 1), (1, 2)], dtype=np.int32)
    for vec, dist, starts in ((raw, None, None), (u, r, np.array([3, 320, 633]))):
        for x, y in zip(oracle_dipolar_fft(vec, dist, R, F, starts), oracle_dipolar(vec, dist, R, F, starts)):
            assert x.shape == y.shape and np.max(np.abs(x - y)) < 1e-12
        for sym in (0, 1):
            for x, y in zip(oracle_dcross_fft(vec, dist, pairs, sym, R, F, starts), oracle_dcross(vec, dist, pairs, sym, R, F, starts)):
                assert x.shape == y.shape and np.max(np.abs(x - y)) < 1e-12


# ---- the identity ------------------------------------------------------------------------------------------------------------------------
def five_signal_core(a4, w4, pairs, sym):
    """C (L, nP) and P0 (nP) from the traceless part of a (x) a alone: c_r(k) = 1.5 sum Q_i : Q_j' / (F - k), the normaliser from w"""
    a4, w4 = np.asarray(a4, dtype=np.float64), np.asarray(w4, dtype=np.float64)
    pairs = np.asarray(pairs)
    R, F = w4.shape[:2]
    L = F // 2
    q = products(a4)
    q[:3] -= ((a4 ** 2).sum(axis=-1) / 3.0)[None]                              # Q = a (x) a - (|a|^2 / 3) I
    qi, qj = q[..., pairs[:, 0]], q[..., pairs[:, 1]]
    S = (G6 * lag_sums(qi, qj, L)).sum(axis=0)
    if sym:
        S = 0.5 * (S + (G6 * lag_sums(qj, qi, L)).sum(axis=0))
    c = 1.5 * S / (F - np.arange(L + 1))[None, :, None]
    n = ((w4 ** 2).sum(axis=1) / F).mean(axis=0)
    m = c.mean(axis=0) / np.sqrt(n[pairs[:, 0]] * n[pairs[:, 1]])
    return m[1:], m[0]


def test_five_traceless_signals_give_the_definition_on_float32_planes():
    F, R, V = 10017, 1, 4
    u, r, raw = make_pairs(R * F, seed=10017, nV=V)
    a, w, _ = planes_of(raw, None)
    a4 = a.astype(np.float32).astype(np.float64).reshape(R, F, V, 3)           # what the pack writes: rounded once to float32
    w4 = w.astype(np.float32).astype(np.float64).reshape(R, F, V)
    pairs = np.array([(0, 0), (1, 1), (2, 2), (3, 3), (1, 2), (3, 1)], dtype=np.int32)
    for sym in (0, 1):
        P0, _, C, _, _ = fft_cross_core(a4, w4, pairs, sym)
        C5, P05 = five_signal_core(a4, w4, pairs, sym)
        assert C.min() >= 0.4 and P0.min() >= 0.4
        print('sym=%d: five signals against the definition %.2e (C), %.2e (P0)' % (sym, relerr(C5, C), relerr(P05, P0)))
        assert relerr(C5, C) < 1e-7 and relerr(P05, P0) < 1e-7
    # the autocorrelation form is the pair (v, v): the same numbers from fft_core
    Ca = fft_core(a4, w4)[0]
    assert np.max(np.abs(Ca - fft_cross_core(a4, w4, pairs[:4], 0)[2])) < 1e-12
    # and on planes in float64, where |a|^2 = w to 1e-16, the identity is exact to rounding
    C, C5 = fft_cross_core(a.reshape(R, F, V, 3), w.reshape(R, F, V), pairs, 1)[2], five_signal_core(a.reshape(R, F, V, 3), w.reshape(R, F, V), pairs, 1)[0]
    assert relerr(C5, C) < 1e-12


# ---- symbols -----------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_new_entry_points():
    with open(os.path.join(ROOT, 'include', 'spinrelax_hip.h')) as fp:
        raw = fp.read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    for name, nargs in NEW.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        m = re.search(r'\b(int|int64_t) %s\((.*?)\);' % name, text, flags=re.S)
        assert m and len(m.group(2).split(',')) == nargs, name
        # the blocked counterpart takes the arguments of the function it stands beside
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace('_long', '')]
        d = re.search(r'\b(int|int64_t) %s\((.*?)\);' % name.replace('_long', ''), text, flags=re.S)
        assert d and ' '.join(d.group(2).split()) == ' '.join(m.group(2).split()) and d.group(1) == m.group(1), name
    for name in ('sr_ct_dipolar_long_max_frames', 'sr_ct_dipolar_cross_long_max_frames'):
        assert _lib.SIGNATURES[name][0] is ctypes.c_int64
    assert 'SR_ABI_VERSION 13' in raw and _lib.ABI_VERSION == 13
    assert 'no blocked form' not in raw


def test_library_exports_the_new_entry_points():
    if not os.path.isfile(_lib.LIB_PATH):
        from spinrelax_amd import build
        build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    assert lib.sr_abi_version() == 13
    assert lib.sr_ct_dipolar_long_max_frames(None) == -1                  # no context: refused on the host, nothing touched
    assert lib.sr_ct_dipolar_cross_long_max_frames(None) == -1


# ---- dispatch ----------------------------------------------------------------------------------------------------------------------------
class StubContext:
    """what ct._dispatch asks of a context for its three stems: the limits of both forms and the three options, kept as hip.Context
    keeps them"""
    ct_cross_long_min_frames = 6625
    ct_dipolar_long_min_frames = 10017
    ct_dipolar_cross_long_min_frames = 4897

    def ct_cross_max_frames(self):
        return 6624

    def ct_cross_long_max_frames(self):
        return 262144

    def ct_dipolar_max_frames(self):
        return 10016

    def ct_dipolar_cross_max_frames(self):
        return 4896

    def ct_dipolar_long_max_frames(self):
        return 262144

    def ct_dipolar_cross_long_max_frames(self):
        return 262144


class StubVectors:
    def __init__(self, nV=3, frames=1 << 20):
        self.ctx, self.nV, self.frames, self.calls = StubContext(), nV, frames, []

    def ct_cross(self, R, F, pairs, **kw):
        self.calls.append(('direct', R, F, kw))
        return 'udirect'

    def ct_cross_long(self, R, F, pairs, **kw):
        self.calls.append(('blocked', R, F, kw))
        return 'ublocked'

    def ct_dipolar(self, R, F, **kw):
        self.calls.append(('direct', R, F, kw))
        return 'direct'

    def ct_dipolar_long(self, R, F, **kw):
        self.calls.append(('blocked', R, F, kw))
        return 'blocked'

    def ct_dipolar_cross(self, R, F, pairs, **kw):
        self.calls.append(('direct', R, F, kw))
        return 'xdirect'

    def ct_dipolar_cross_long(self, R, F, pairs, **kw):
        self.calls.append(('blocked', R, F, kw))
        return 'xblocked'


def test_dispatch_of_the_dipolar_correlation_function():
    rv = StubVectors()
    assert hostct.calculate_Ct_dipolar_resident(rv, 2, 10016) == 'direct'
    assert hostct.calculate_Ct_dipolar_resident(rv, 2, 10017, chunk_start=[0, 10017], mode=1) == 'blocked'
    assert rv.calls[-1] == ('blocked', 2, 10017, {'dist': None, 'chunk_start': [0, 10017], 'mode': 1})
    assert hostct.calculate_Ct_dipolar_resident(rv, 1, 262144) == 'blocked'
    with pytest.raises(ValueError) as exc:
        hostct.calculate_Ct_dipolar_resident(rv, 1, 262145)
    assert '10016' in str(exc.value) and '262144' in str(exc.value)
    rv.ctx.ct_dipolar_long_min_frames = 5462
    assert hostct.calculate_Ct_dipolar_resident(rv, 2, 5461) == 'direct'
    assert hostct.calculate_Ct_dipolar_resident(rv, 2, 5462) == 'blocked'
    assert hostct.calculate_Ct_dipolar_resident(rv, 2, 10016) == 'blocked'


def test_dispatch_of_the_dipolar_pair_cross_correlation():
    rv = StubVectors()
    pairs = [(0, 1), (2, 2)]
    assert hostct.calculate_Ct_dipolar_cross_resident(rv, pairs, 2, 4896) == 'xdirect'
    assert hostct.calculate_Ct_dipolar_cross_resident(rv, pairs, 2, 4897, symmetric=False) == 'xblocked'
    assert rv.calls[-1] == ('blocked', 2, 4897, {'dist': None, 'chunk_start': None, 'sym': 0, 'mode': 0})
    assert hostct.calculate_Ct_dipolar_cross_resident(rv, pairs, 1, 262144) == 'xblocked'
    with pytest.raises(ValueError) as exc:
        hostct.calculate_Ct_dipolar_cross_resident(rv, pairs, 1, 262145)
    assert '4896' in str(exc.value) and '262144' in str(exc.value)
    rv.ctx.ct_dipolar_cross_long_min_frames = 4097
    assert hostct.calculate_Ct_dipolar_cross_resident(rv, pairs, 2, 4096) == 'xdirect'
    assert hostct.calculate_Ct_dipolar_cross_resident(rv, pairs, 2, 4097) == 'xblocked'
    assert hostct.calculate_Ct_dipolar_cross_resident(rv, pairs, 2, 4896) == 'xblocked'


def test_dispatch_of_the_pair_cross_correlation():
    rv = StubVectors()
    pairs = [(0, 1), (2, 2)]
    assert hostct.calculate_Ct_cross_resident(rv, pairs, 2, 6624) == 'udirect'
    assert hostct.calculate_Ct_cross_resident(rv, pairs, 2, 6625, symmetric=False, want_dP0=True) == 'ublocked'
    assert rv.calls[-1] == ('blocked', 2, 6625, {'chunk_start': None, 'sym': 0, 'mode': 0, 'want_dP0': True})
    assert hostct.calculate_Ct_cross_resident(rv, pairs, 1, 262144) == 'ublocked'
    with pytest.raises(ValueError) as exc:
        hostct.calculate_Ct_cross_resident(rv, pairs, 1, 262145)
    assert '6624' in str(exc.value) and '262144' in str(exc.value)
    rv.ctx.ct_cross_long_min_frames = 5462
    assert hostct.calculate_Ct_cross_resident(rv, pairs, 2, 5461) == 'udirect'
    assert hostct.calculate_Ct_cross_resident(rv, pairs, 2, 5462) == 'ublocked'
    assert hostct.calculate_Ct_cross_resident(rv, pairs, 2, 6624) == 'ublocked'


# stem, label of the error text, staged limit, floor of the blocked form, extra positional arguments, names of the two forms' results
STEMS = [('cross', 'cross-correlation functions', 6624, 5462, ([(0, 1)],), ('udirect', 'ublocked')),
         ('dipolar', 'dipolar correlation function', 10016, 5462, (), ('direct', 'blocked')),
         ('dipolar_cross', 'dipolar cross-correlation functions', 4896, 4097, ([(0, 1)],), ('xdirect', 'xblocked'))]


@pytest.mark.parametrize('stem,label,staged,floor,extra,names', STEMS)
def test_one_dispatch_rule_for_the_three_stems(stem, label, staged, floor, extra, names):
    """ct._dispatch at the staged limit, one beyond it, the floor the option may be set to, the blocked limit and one beyond it: the
    decisions of the three functions it replaced (beyond the staged limit or from the option on: blocked; beyond both: ValueError with the
    text of that function, word for word)"""
    rv = StubVectors()
    go = lambda F: hostct._dispatch(rv, stem, label, F, 2, F, *extra, mode=1)
    assert go(staged) == names[0] and rv.calls[-1] == ('direct', 2, staged, {'mode': 1})
    assert go(staged + 1) == names[1] and rv.calls[-1] == ('blocked', 2, staged + 1, {'mode': 1})
    assert go(262144) == names[1]
    with pytest.raises(ValueError) as exc:
        go(262145)
    assert str(exc.value) == ('%s: a chunk of 262145 frames is beyond both forms (the staged kernel takes %d frames, the blocked transforms '
                              '262144)' % (label, staged))
    assert len(rv.calls) == 3                                             # the refusal called neither form
    setattr(rv.ctx, 'ct_%s_long_min_frames' % stem, floor)
    assert go(floor - 1) == names[0] and go(floor) == names[1] and go(staged) == names[1]


def test_no_source_claims_that_a_blocked_form_is_missing():
    """every staged form names its blocked counterpart in its -4 message (tests/test_gpu_ct_cross.py holds the library to it)"""
    for sub in (os.path.join('spinrelax_amd', 'csrc'), 'include'):
        for name in sorted(os.listdir(os.path.join(ROOT, sub))):
            if name.endswith(('.hip', '.h')):
                with open(os.path.join(ROOT, sub, name)) as fp:
                    assert 'no blocked form' not in fp.read(), name


def test_context_keeps_the_defaults_of_the_two_options():
    from spinrelax_amd.hip import Context
    assert Context.ct_dipolar_long_min_frames == 10017 and Context.ct_dipolar_cross_long_min_frames == 4897
    for name in ('ct_dipolar_long_max_frames', 'ct_dipolar_cross_long_max_frames', 'ct_dipolar_long_dev', 'ct_dipolar_cross_long_dev'):
        assert callable(getattr(Context, name))
