"""
Host side of the iRED mode correlation functions (spinrelax_amd/ired.py, the --iRED_Ct flag, the ABI declarations): no GPU.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from spinrelax_amd import _lib, ired


def test_mode_tau_closed_form():
    """lambda exp(-k dt / tau): the trapezoid sum of r^k, k < n, is (1 - r^n) / (1 - r) - (1 + r^(n-1)) / 2"""
    dt, n = 2.0, 400
    k = np.arange(n)
    for lam, tau in ((0.7, 35.0), (3.0, 5.0), (1e-4, 900.0)):
        r = np.exp(-dt / tau)
        ref = dt * ((1.0 - r ** n) / (1.0 - r) - 0.5 * (1.0 + r ** (n - 1)))
        got = ired.ired_mode_tau(lam * np.exp(-k * dt / tau), dt)
        assert abs(got - ref) <= 1e-12 * ref, (lam, tau)
    both = ired.ired_mode_tau(np.stack((0.7 * np.exp(-k * dt / 35.0), 3.0 * np.exp(-k * dt / 5.0))), dt)
    assert both.shape == (2,) and both[0] > both[1] > 0.0


def test_mode_tau_truncation_and_dead_modes():
    C = np.array([[1.0, 0.5, 0.25, -0.1, 0.3],        # the sum stops before the first value <= 0: lags 0 .. 2
                  [2.0, 1.0, 0.0, 5.0, 5.0],          # an exact zero ends it too
                  [0.0, 1.0, 1.0, 1.0, 1.0],          # C(0) = 0
                  [-1.0, 1.0, 1.0, 1.0, 1.0],
                  [4.0, 0.0, 0.0, 0.0, 0.0]])         # only lag 0 is left: a trapezoid of no width
    tau = ired.ired_mode_tau(C, 3.0)
    assert np.allclose(tau, [3.0 * (1.75 - 0.625), 3.0 * (1.5 - 0.75), 0.0, 0.0, 0.0], rtol=1e-15, atol=0.0)


def test_vector_ct_against_a_loop():
    rng = np.random.default_rng(5)
    vec, Cm = rng.standard_normal((3, 7, 7)), rng.standard_normal((3, 7, 11))
    got = ired.ired_vector_ct(vec, Cm)
    assert got.shape == (3, 7, 11)
    for w in range(3):
        for i in range(7):
            for k in range(11):
                ref = sum(vec[w, i, m] ** 2 * Cm[w, m, k] for m in range(7))
                assert abs(got[w, i, k] - ref) < 1e-13
    assert np.array_equal(ired.ired_vector_ct(vec[0], Cm[0]), got[0])
    with pytest.raises(ValueError):
        ired.ired_vector_ct(vec[0][:, :5], Cm[0])


def test_S2_modes_is_ired_S2_with_the_eigenvectors_as_rows():
    rng = np.random.default_rng(9)
    a = rng.standard_normal((2, 9, 9))
    M = a + np.swapaxes(a, 1, 2)
    S2, lam = ired.ired_S2(M, 5)
    S2b, lamb, modes = ired.ired_S2_modes(M, 5)
    assert S2.tobytes() == S2b.tobytes() and lam.tobytes() == lamb.tobytes()
    for w in range(2):
        assert np.max(np.abs(M[w] @ modes[w].T - modes[w].T * lam[w])) < 1e-12
        assert np.all(np.diff(lam[w]) <= 0.0)


class _NoGpu(Exception):
    pass


class _StubVectors:
    nV = 24

    def ired(self, *a):
        raise _NoGpu()

    ired_mode_ct = ired


def test_window_too_long_is_refused_before_any_launch():
    stub = _StubVectors()
    with pytest.raises(ValueError) as exc:
        ired.calculate_iRED_resident(stub, [12000], 1.0, window=5462.0, mode_ct=True)
    assert '--iRED_window' in str(exc.value) and '5461' in str(exc.value)
    with pytest.raises(ValueError):
        ired.calculate_iRED_resident(stub, [12000], 1.0, window=5000.0, mode_ct=True, n_lags=3194)      # 5000 + 3193 = 8193
    with pytest.raises(ValueError):
        ired.calculate_iRED_resident(stub, [700, 900], 1.0, mode_ct=True)                                # whole files: two lengths
    with pytest.raises(ValueError):
        ired.calculate_iRED_resident(stub, [700], 1.0, mode_ct=True, n_lags=701)
    # the boundary itself passes the checks and reaches the GPU calls
    with pytest.raises(_NoGpu):
        ired.calculate_iRED_resident(stub, [12000], 1.0, window=5461.0, mode_ct=True)
    with pytest.raises(_NoGpu):
        ired.calculate_iRED_resident(stub, [12000], 1.0, window=5000.0, mode_ct=True, n_lags=3193)


def test_iRED_Ct_alone_is_refused():
    script = os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')
    p = subprocess.run([sys.executable, script, '-s', 'none.pdb', '-f', 'none.npy', '--iRED_Ct'], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert p.returncode != 0
    assert b'--iRED' in p.stderr and b'Traceback' not in p.stderr


def test_abi_declares_the_new_entry_points():
    for name in ('sr_ired_mode_ct_f32_dev', 'sr_vectors_ired_mode_ct_f32'):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['sr_ired_mode_ct_f32_dev'][1]) == 11 and len(_lib.SIGNATURES['sr_vectors_ired_mode_ct_f32'][1]) == 9
    with open(os.path.join(ROOT, 'include', 'spinrelax_hip.h')) as fp:
        text = fp.read()
    assert _lib.ABI_VERSION == 13 == int(re.search(r'#define SR_ABI_VERSION (\d+)', text).group(1))
    for name in ('sr_ired_mode_ct_f32_dev', 'sr_vectors_ired_mode_ct_f32'):
        assert re.search(r'\bint %s\(sr_ctx \*' % name, text)
