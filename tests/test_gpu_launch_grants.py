"""
GPU tests of the dynamic-LDS grants above 64 KiB (sr_launch / sr_grant_lds, sr_internal.h and sr_core.hip).  The attribute that
allows such a launch belongs to ONE function on one device: every instance of a kernel template needs its own grant, a smaller
request must not lower a larger one, and a second context on the same device must not lower the first one's.  The shapes are the
smallest that reach each grant: fit residues that just cross 64 KiB in LDS, and one chunk length per C(t) transform length.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, relerr
from spinrelax_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from spinrelax_amd.hip import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def liboracle():
    so = os.path.join(ROOT, 'oracle', 'libsr_oracle.so')
    if not os.path.isfile(so):
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'oracle'), 'libsr_oracle.so'])
    lib = ctypes.CDLL(so)
    lib.sr_oracle_ct_palmer_f64.restype = ctypes.c_int
    return lib


def c_oracle_ct(lib, v4):
    v4 = np.ascontiguousarray(v4, dtype=np.float32)
    R, F, V, _ = v4.shape
    L = F // 2
    Ct = np.empty((L, V))
    dCt = np.empty((L, V))
    rc = lib.sr_oracle_ct_palmer_f64(v4.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(R), ctypes.c_int64(F),
                                     ctypes.c_int64(V), Ct.ctypes.data_as(ctypes.c_void_p),
                                     dCt.ctypes.data_as(ctypes.c_void_p), None)
    assert rc == 0
    return Ct, dCt


def biexp(L, nRes=2):
    """bi-exponential decays on a uniform grid, the time constants of spinrelax_amd.synth, mild noise"""
    rng = np.random.RandomState(L)
    t = synth.DT_PS * np.arange(1, L + 1)
    y = np.empty((nRes, L))
    for i in range(nRes):
        C1, C2 = 0.10 + 0.02 * i, 0.15 - 0.02 * i
        y[i] = (1.0 - C1 - C2) + C1 * np.exp(-t / synth.TAUS_PS[0]) + C2 * np.exp(-t / synth.TAUS_PS[1])
    y += 1e-4 * rng.standard_normal(y.shape)
    return np.broadcast_to(t, (nRes, L)).copy(), y, np.full((nRes, L), 1e-3)


def p0_of(P, nRes=2):
    K = P // 2
    return np.tile(np.concatenate([np.full(K, 0.5 / K), 30.0 * 8.0 ** np.arange(K)]), (nRes, 1))


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_fit_grants_per_function_and_across_contexts(ctx):
    """fit_waves = 4: a residue staged in LDS takes 8 (1000 + 2 L) bytes, above 64 KiB from L = 3 730.  P = 4 at L = 4200, then
    P = 6 at the same size (another function of the same template), then P = 4 at L = 3800 (smaller, still above 64 KiB), then
    P = 4 at L = 4200 from a second context on the device and again from the first: every launch succeeds and the three
    P = 4, L = 4200 fits (popt, pcov, chisq, status, nfev) are bit-identical.  The model-order search likewise."""
    from spinrelax_amd.hip import Context
    big, small = biexp(4200), biexp(3800)
    tau_max = 10.0 * big[0][0, -1]
    other = None
    ctx.set_option('fit_waves', 4)
    try:
        first = ctx.expfit(*big, p0_of(4), tau_max)
        ctx.expfit(*big, p0_of(6), tau_max)
        ctx.expfit(*small, p0_of(4), tau_max)
        other = Context(0)
        other.set_option('fit_waves', 4)
        second = other.expfit(*big, p0_of(4), tau_max)
        third = ctx.expfit(*big, p0_of(4), tau_max)
        assert same(first, second) and same(first, third)

        tg = np.array([[100.0, 30.0, 500.0]])
        keys = ('popt', 'dP', 'chisq', 'status', 'nfev', 'best', 'S2', 'C', 'tau', 'chi', 'K')
        s1 = ctx.order_search(*big, (2, 4), tg, tau_max)
        ctx.order_search(*small, (2, 4), tg, tau_max)
        s3 = ctx.order_search(*big, (2, 4), tg, tau_max)
        assert same([s1[k] for k in keys], [s3[k] for k in keys])
    finally:
        ctx.set_option('fit_waves', 2)
        if other is not None:
            other.close()


def test_ct_transform_grants(ctx, liboracle):
    """The float64 C(t) transforms above 64 KiB of LDS.  ct_fft = 1 at F + L > 4096 runs k_ct_fft<32> (F = 5000, M = 8192) and
    k_ct_fft<24> (F = 3000, M = 6144); ct_fft = 2 at F = 5000 runs k_ct_rfft<16>.  Large, smaller, large again: each against the
    plain-C float64 oracle within the float64 bars of test_ct_fft_formulation_all_transform_sizes (ct_fft = 2), and the two
    F = 5000, ct_fft = 1 results bit-identical."""
    R, V = 2, 2
    data = {}
    for F in (5000, 3000):
        vecs = synth.synth_vectors(R * F + 5, V, seed=300 + F)
        data[F] = (vecs, c_oracle_ct(liboracle, vecs[:R * F].reshape(R, F, V, 3)))
    got = []
    try:
        for ct_fft, F in ((1, 5000), (1, 3000), (1, 5000), (2, 5000)):
            ctx.set_option('ct_fft', ct_fft)
            got.append((ct_fft, F) + ctx.ct_palmer(data[F][0], R, F))
    finally:
        ctx.set_option('ct_fft', 3)
    for ct_fft, F, Ct, dCt in got:
        Cr, dCr = data[F][1]
        assert Ct.shape == (F // 2, V)
        assert relerr(Ct, Cr) < 1e-12, (ct_fft, F, relerr(Ct, Cr))
        assert np.max(np.abs(dCt - dCr)) <= 1e-12 * max(1.0, np.max(np.abs(dCr))), (ct_fft, F)
    assert np.array_equal(got[0][2], got[2][2]) and np.array_equal(got[0][3], got[2][3])
