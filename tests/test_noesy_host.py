"""
CPU tests of the NOESY layer (spinrelax_amd/noesy.py, csrc/sr_noesy.hip): the scaling arithmetic of the matrix exponential pinned by
literals, the group sum on a 5-spin example worked by hand, the _noesy.dat round trip, the flag refusals of the script before any GPU
work, and the ctypes signatures.  Nothing here touches a GPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _built():
    from spinrelax_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        from spinrelax_amd import build
        build.build(verbose=False)


def test_symm_expm_plan_literals():
    """s = the least integer >= 0 with norm1 tau / 2^s <= 0.5, products = 11 + s (Horner of degree 12, then s squarings): written out
    by hand, not recomputed.  Both sides of the threshold, the exact powers of two, zero, and the refusals."""
    _built()
    from spinrelax_amd import hip
    from spinrelax_amd._lib import SpinRelaxHipError
    cases = [((0.0, 0.3), (0, 11)), ((5.0, 0.0), (0, 11)), ((1.0, 0.5), (0, 11)), ((1.0, 0.5000001), (1, 12)), ((1.0, 1.0), (1, 12)),
             ((2.0, 1.0), (2, 13)), ((100.0, 0.2), (6, 17)),            # 20 / 32 = 0.625, 20 / 64 = 0.3125
             ((110.0, 0.8), (8, 19)),                                   # 88 / 128 = 0.6875, 88 / 256 = 0.34
             ((128.0, 1.0), (8, 19)), ((128.0, 1.0000001), (9, 20)),
             ((2.0 ** 39, 1.0), (40, 51))]
    for (n1, tau), want in cases:
        assert hip.symm_expm_plan(n1, tau) == want, (n1, tau)
    assert hip.Context.symm_expm_plan(100.0, 0.2) == (6, 17)          # the same function, reachable from the class
    for n1, tau, msg in ((2.0 ** 40, 1.0, 'more than 40 squarings'), (1.0, -0.1, 'mixing time'), (np.inf, 1.0, 'not finite'),
                         (np.nan, 1.0, 'not finite'), (1.0, np.nan, 'mixing time'), (-1.0, 1.0, 'not finite')):
        with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_symm_expm_plan: .*' + msg):
            hip.symm_expm_plan(n1, tau)


def test_sum_groups_five_spins_by_hand():
    """A_ij = 10 i + j + 1 (not symmetric, so a transposed sum would show).  Groups: a methyl {0, 1, 2}, and the singles {3}, {4}.
      G0-G0: rows 0, 1, 2 x columns 0, 1, 2: (1 + 2 + 3) + (11 + 12 + 13) + (21 + 22 + 23) = 108
      G0-G1: column 3: 4 + 14 + 24 = 42;    G0-G2: column 4: 5 + 15 + 25 = 45
      G1-G0: row 3: 31 + 32 + 33 = 96;      G1-G1: 34;   G1-G2: 35
      G2-G0: row 4: 41 + 42 + 43 = 126;     G2-G1: 44;   G2-G2: 45"""
    from spinrelax_amd import noesy
    A = 10.0 * np.arange(5)[:, None] + np.arange(5)[None, :] + 1.0
    want = np.array([[108.0, 42.0, 45.0], [96.0, 34.0, 35.0], [126.0, 44.0, 45.0]])
    got = noesy.sum_groups(A, [[0, 1, 2], [3], [4]])
    assert np.array_equal(got, want)
    # a stack of matrices, groups in another order and one spin left out
    got2 = noesy.sum_groups(np.stack([A, 2 * A]), [[4], [2, 0]])
    assert got2.shape == (2, 2, 2)
    assert np.array_equal(got2[0], [[45.0, 41.0 + 43.0], [5.0 + 25.0, 1.0 + 3.0 + 21.0 + 23.0]]) and np.array_equal(got2[1], 2 * got2[0])
    for bad, msg in (([[0, 5]], 'outside'), ([[0, 1], [1]], 'twice'), ([[0, 0]], 'twice'), ([[]], 'empty')):
        with pytest.raises(ValueError, match=msg):
            noesy.sum_groups(A, bad)


def test_write_read_round_trip(tmp_path):
    from spinrelax_amd import noesy
    from spinrelax_amd.noe import n_pairs, pair_list
    rng = np.random.default_rng(5)
    P, tau = 4, np.array([0.0, 0.05, 0.2])
    idx = np.array([3, 7, 8, 12])
    R = rng.standard_normal((P, P))
    R = R + R.T
    A = rng.uniform(-1, 1, (tau.size, P, P))
    A = A + A.transpose(0, 2, 1)
    res = dict(index=idx, R=R, A=A, mixing_times=tau)
    fn = str(tmp_path / 'o_noesy.dat')
    names = ['H%d' % a for a in idx]
    assert noesy.write_noesy(fn, res, names=names) == P + n_pairs(P)
    with open(fn) as fp:
        head = fp.readline()
    assert head == '# i j name_i name_j sigma A0 A1 A2\n'
    tab = noesy.read_noesy(fn)
    ii, jj = np.triu_indices(P)                                   # rows: i <= j, row-major, the diagonal included
    assert np.array_equal(tab['i'], idx[ii]) and np.array_equal(tab['j'], idx[jj])
    assert tab['name_i'] == [names[i] for i in ii] and tab['name_j'] == [names[j] for j in jj]
    assert np.array_equal(tab['mixing_times'], tau)
    assert np.max(np.abs(tab['sigma'] - R[ii, jj]) / np.abs(R[ii, jj])) <= 5e-8         # %.8g
    assert tab['A'].shape == (ii.size, 3) and np.max(np.abs(tab['A'] - A[:, ii, jj].T)) <= 5e-8 * 2
    # a cutoff on reff6 drops pairs and never a diagonal row
    reff6 = np.arange(n_pairs(P), dtype=np.float64)
    assert noesy.write_noesy(fn, res, reff6=reff6, cutoff=2.0) == P + 3
    tab = noesy.read_noesy(fn)
    kept = pair_list(P)[:3]
    off = tab['i'] != tab['j']
    assert np.array_equal(tab['i'][off], idx[kept[:, 0]]) and np.array_equal(tab['j'][off], idx[kept[:, 1]]) and (~off).sum() == P
    with pytest.raises(ValueError, match='needs reff6'):
        noesy.write_noesy(fn, res, cutoff=2.0)
    with pytest.raises(ValueError, match='white space'):
        noesy.write_noesy(fn, res, names=['a b', 'c', 'd', 'e'])


def test_prefactor_and_units():
    """q = 0.1 (mu0 / 4 pi)^2 hbar^2 gamma_H^4 from the CODATA values, and its two coordinate units"""
    from spinrelax_amd import noesy
    mu0_4pi, hbar, gH = 1e-7, 1.054571817e-34, 267.513e6
    assert abs(noesy.Q_HH / (0.1 * mu0_4pi ** 2 * hbar ** 2 * gH ** 4) - 1) < 1e-6
    assert abs(noesy.prefactor('A') / (noesy.Q_HH * 1e60) - 1) < 1e-12 and abs(noesy.prefactor('nm') / (noesy.Q_HH * 1e54) - 1) < 1e-12
    assert abs(noesy.prefactor('nm') / noesy.prefactor(1e-9) - 1) < 1e-15
    assert abs(noesy.omega_H(600.0) - 2 * np.pi * 6e8) < 1.0


def test_cli_flag_refusals_without_gpu(tmp_path):
    """Every combination of --noesy* flags that does not fit together ends in the script's '= = = ERROR:' message and exit status 1
    before any GPU work: this machine has no GPU and the input file does not even exist."""
    script = os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')
    base = [sys.executable, script, '-s', 'none.pdb', '-f', str(tmp_path / 'missing.npz'), '-o', str(tmp_path / 'o')]
    full = ['--noesyMix', '0.05 0.1', '--noesyField', '600', '--noesyTauC', '5e-9']
    cases = [(['--noesyMix', '0.1'], '--noesyMix belongs to --noesy'),
             (['--noeMap', '--noesyField', '600'], '--noesyField belongs to --noesy'),
             (['--noesyTauC', '5e-9'], '--noesyTauC belongs to --noesy'),
             (['--noesyTauE', '1e-10'], '--noesyTauE belongs to --noesy'),
             (['--noesyLeak', '0.5'], '--noesyLeak belongs to --noesy'),
             (['--noesyUnit', 'A'], '--noesyUnit belongs to --noesy'),
             (['--noesyGroups', 'g.txt'], '--noesyGroups belongs to --noesy'),
             (['--noesy'] + full, '--noesy works on the map of --noeMap'),
             (['--noeMap', '--noesy', '--noesyMix', '0.1', '--noesyTauC', '5e-9'], '--noesy needs --noesyField'),
             (['--noeMap', '--noesy', '--noesyMix', '0.1', '--noesyField', '600'], '--noesy needs --noesyTauC'),
             (['--noeMap', '--noesy', '--noesyField', '600', '--noesyTauC', '5e-9'], '--noesy needs --noesyMix'),
             (['--noeMap', '--noesy', '--noesyMix', '0.1 x', '--noesyField', '600', '--noesyTauC', '5e-9'], '--noesyMix must list'),
             (['--noeMap', '--noesy', '--noesyMix', '-0.1', '--noesyField', '600', '--noesyTauC', '5e-9'], '--noesyMix must list'),
             (['--noeMap', '--noesy', '--noesyMix', '0.1', '--noesyField', '600', '--noesyTauC', '0'], 'must be > 0'),
             (['--noeMap', '--noesy'] + full + ['--noesyGroups', str(tmp_path / 'nogroups.txt')], 'does not exist')]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for extra, msg in cases:
        p = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
        err = p.stderr.decode()
        assert p.returncode == 1 and ('= = = ERROR: ' in err) and msg in err, (extra, p.returncode, err[-500:])
        assert not os.listdir(str(tmp_path))


def test_signatures_present():
    _built()
    from ctypes import c_double, c_int64, c_void_p
    from spinrelax_amd import _lib
    names = ('sr_noesy_rates_f64_dev', 'sr_noesy_rates_f64', 'sr_symm_mul_f64_dev', 'sr_symm_expm_f64_dev', 'sr_symm_expm_plan',
             'sr_symm_expm_check')
    for n in names:
        assert n in _lib.SIGNATURES, n
    lib = _lib.load()
    for n in names:
        assert getattr(lib, n).argtypes == _lib.SIGNATURES[n][1]
    assert _lib.SIGNATURES['sr_symm_mul_f64_dev'][1] == [c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double, c_void_p]
    assert _lib.SIGNATURES['sr_noesy_rates_f64'][1][5:11] == [c_int64] + [c_double] * 5
    assert _lib.ABI_VERSION == 13 and lib.sr_abi_version() == 13


def test_device_functions_raise_without_gpu():
    """no CPU fallback: on a machine without a GPU every device function raises SpinRelaxHipError"""
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    _built()
    from spinrelax_amd import noesy
    from spinrelax_amd._lib import SpinRelaxHipError
    m = dict(A6=np.ones(3), S2=np.full(3, 0.8), index=np.arange(3))
    with pytest.raises(SpinRelaxHipError):
        noesy.rate_matrix(m, 600.0, 5e-9)
    with pytest.raises(SpinRelaxHipError):
        noesy.intensities(np.eye(3), [0.1])
    with pytest.raises(SpinRelaxHipError):
        noesy.noesy(m, [0.1], 600.0, 5e-9)
