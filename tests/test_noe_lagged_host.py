"""
CPU tests of the lagged dipolar map's host side (spinrelax_amd/noe.py, noesy.py, csrc/sr_noe.hip's symbols): the Lipari-Szabo
integral tau_e_from_Cdd on a known decay and against a plain loop, log_lags, the _noeMapCt.dat round trip, Cdd and dCdd assembled from
hand-made G with ragged blocks, the tau_e='map' floor and refusal, the script's flag refusals before any GPU work, and the ctypes
signatures.  Nothing here touches a GPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from spinrelax_amd import noe, noesy


def _built():
    from spinrelax_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        from spinrelax_amd import build
        build.build(verbose=False)


def loop_tau_e(C, S2, lags, dt):
    """the rule of tau_e_from_Cdd as a plain loop over one series: trapezoids of y = (C - S2) / (1 - S2) through (0, 1) and the given
    points, up to the first point with C <= S2, where the line from the last point crosses zero; 0 for a rigid pair"""
    if 1.0 - S2 < 1e-6:
        return 0.0
    t0, y0, area = 0.0, 1.0, 0.0
    for k, c in zip(lags, C):
        if k == 0:
            continue
        t1, y1 = float(k), (c - S2) / (1.0 - S2)
        if c <= S2:
            tc = t0 + (t1 - t0) * y0 / (y0 - y1)
            return (area + 0.5 * y0 * (tc - t0)) * dt
        area += 0.5 * (y0 + y1) * (t1 - t0)
        t0, y0 = t1, y1
    return area * dt


def test_tau_e_recovers_an_exponential():
    """C(k) = S2 + (1 - S2) exp(-k / 5) at the lags 0 .. 50: the integral is 5 (1 - e^-10), the trapezoid rule at unit spacing
    overestimates it by (1 / 12) / tau^2 = 0.33 %: within 1 % of 5; in the units of dt"""
    k = np.arange(51)
    for S2 in (0.0, 0.3, 0.85):
        C = S2 + (1 - S2) * np.exp(-k / 5.0)
        tau = noe.tau_e_from_Cdd(C, S2, k, 1.0)
        assert abs(tau / 5.0 - 1) <= 0.01, (S2, tau)
        assert noe.tau_e_from_Cdd(C[1:], S2, k[1:], 1.0) == tau                    # a given lag 0 is replaced by (0, 1)
        assert noe.tau_e_from_Cdd(C, S2, k, 2.5e-12) == tau * 2.5e-12              # dt multiplies the finished integral
    # many pairs at once, (K, n)
    S2 = np.array([0.1, 0.5, 0.9])
    C = S2[None] + (1 - S2[None]) * np.exp(-k[:, None] / 5.0)
    tau = noe.tau_e_from_Cdd(C, S2, k, 2.0)
    assert tau.shape == (3,) and np.all(np.abs(tau / 10.0 - 1) <= 0.01)


def test_tau_e_crossing_and_rigid_rules_against_a_loop():
    """hand-made series: one that never reaches S2, one that crosses between two lags (the integral stops at the interpolated
    crossing and ignores the later recovery), one that sits ON S2 at a lag (C <= S2 stops there), one below S2 at the first lag, a
    rigid pair (1 - S2 < 1e-6) and a pair just on the flexible side of that rule"""
    lags = np.array([1, 2, 4, 8, 16])
    S2 = np.array([0.5, 0.5, 0.5, 0.5, 1.0 - 5e-7, 1.0 - 2e-6])
    C = np.array([[0.9, 0.8, 0.7, 0.6, 0.55],
                  [0.9, 0.7, 0.4, 0.8, 0.9],
                  [0.9, 0.7, 0.5, 0.9, 0.9],
                  [0.3, 0.9, 0.9, 0.9, 0.9],
                  [0.9999999, 0.9999998, 0.9999997, 0.9999996, 0.9999996],
                  [0.999999, 0.9999985, 0.999998, 0.9999975, 0.999997]]).T
    got = noe.tau_e_from_Cdd(C, S2, lags, 0.5)
    want = np.array([loop_tau_e(C[:, n], S2[n], lags, 0.5) for n in range(S2.size)])
    assert got.shape == want.shape and np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (got, want)
    # by hand, dt = 0.5.  Series 1: y = 1, .8, .4, -.2: 0.9 + 0.6 + the triangle to the crossing at 2 + 2 * .4 / .6: 0.5 * .4 * 4 / 3
    assert abs(got[1] - 0.5 * (0.9 + 0.6 + 0.5 * 0.4 * 4.0 / 3.0)) <= 1e-12
    # series 2: y = 1, .8, .4, 0: the last segment is the triangle 0.5 * .4 * 2
    assert abs(got[2] - 0.5 * (0.9 + 0.6 + 0.4)) <= 1e-12
    # series 3: y(1) = -0.4: the triangle from (0, 1) to the crossing at 1 / 1.4
    assert abs(got[3] - 0.5 * 0.5 / 1.4) <= 1e-12
    assert got[4] == 0.0 and got[5] > 0.0
    with pytest.raises(ValueError, match='strictly increasing'):
        noe.tau_e_from_Cdd(C, S2, [1, 2, 2, 8, 16])
    with pytest.raises(ValueError, match='Cdd'):
        noe.tau_e_from_Cdd(C[:3], S2, lags)


def test_log_lags_properties():
    for max_lag, n in ((2048, 12), (1000, 12), (5, 12), (50, 2), (17, 5), (1, 1), (1, 4), (100000, 64)):
        lg = noe.log_lags(max_lag, n)
        assert lg.dtype == np.int64 and lg.ndim == 1 and 1 <= lg.size <= n
        assert lg[0] == 1 and lg[-1] == max_lag and np.all(np.diff(lg) > 0)
        if lg.size > 2 and max_lag >= 4 * n:                  # about log-spaced: neighbouring ratios within a factor of 2 of each other
            ratio = lg[1:] / lg[:-1]
            assert ratio.max() / ratio.min() <= 2.0, (max_lag, n, lg)
    assert noe.log_lags(2048, 12).tolist() == [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048]
    assert noe.log_lags(5, 12).tolist() == [1, 2, 3, 4, 5]
    for bad in ((0, 5), (10, 0), (10, 1)):
        with pytest.raises(ValueError):
            noe.log_lags(*bad)


def _hand_map(rng, bl, lags, P=4):
    """finalize()'s dict of random sums and a G to go with it"""
    npairs = noe.n_pairs(P)
    B = len(bl)
    sums = np.zeros((B, npairs, 7))
    u = rng.standard_normal((B, npairs, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    r3 = rng.uniform(1.0, 2.0, (B, npairs))
    for b in range(B):
        sums[b, :, 0] = bl[b] * r3[b] ** 2 * 1.1
        for k, (a, c) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
            sums[b, :, 1 + k] = bl[b] * r3[b] * u[b, :, a] * u[b, :, c] * 0.9
    fin = noe.finalize(sums, bl)
    G = np.empty((B, len(lags), npairs))
    for b in range(B):
        for q, k in enumerate(lags):
            G[b, q] = (bl[b] - k) * fin['A6_b'][b] * (fin['S2_b'][b] + (1 - fin['S2_b'][b]) * np.exp(-k / (3.0 + b)))
    return sums, fin, G


def test_Cdd_and_dCdd_from_hand_made_G_with_ragged_blocks():
    """three blocks of 37, 20 and 40 frames, lags 0, 1, 5, 19: Cdd = [sum_b G_b(k) / sum_b (n_b - k)] / A6 with its own count of
    origins per lag, the per-block values G_b(k) / (n_b - k) / A6_b, dCdd = std(ddof = 0) / (sqrt(3) - 1), tau_e from the totals and
    dtau_e from the per-block values with each block's own S2_b -- all recomputed here with loops"""
    rng = np.random.default_rng(3)
    bl, lags = [37, 20, 40], [0, 1, 5, 19]
    sums, fin, G = _hand_map(rng, bl, lags)
    out = noe.finalize_lagged(G, bl, lags, fin, dt=2.0)
    npairs = G.shape[2]
    assert out['lags'].tolist() == lags and out['G'] is not None and out['Cdd'].shape == (4, npairs) and out['dCdd'].shape == (4, npairs)
    for q, k in enumerate(lags):
        terms = sum(n - k for n in bl)
        assert terms == (97 - 3 * k)
        want = sum(G[b, q] for b in range(3)) / terms / fin['A6']
        assert np.max(np.abs(out['Cdd'][q] - want)) <= 1e-14
        per = np.stack([G[b, q] / (bl[b] - k) / fin['A6_b'][b] for b in range(3)])
        assert np.max(np.abs(out['Cdd_b'][:, q] - per)) <= 1e-14
        assert np.max(np.abs(out['dCdd'][q] - per.std(axis=0) / (np.sqrt(3.0) - 1))) <= 1e-14
    # per block the hand-made G is S2_b + (1 - S2_b) exp(-k / (3 + b)) exactly
    for b in range(3):
        for q, k in enumerate(lags):
            assert np.max(np.abs(out['Cdd_b'][b, q] - (fin['S2_b'][b] + (1 - fin['S2_b'][b]) * np.exp(-k / (3.0 + b))))) <= 1e-13
    for n in range(npairs):
        assert abs(out['tau_e'][n] - loop_tau_e(out['Cdd'][:, n], fin['S2'][n], lags, 2.0)) <= 1e-12
        per = np.array([loop_tau_e(out['Cdd_b'][b, :, n], fin['S2_b'][b, n], lags, 2.0) for b in range(3)])
        assert np.max(np.abs(out['tau_e_b'][:, n] - per)) <= 1e-12
        assert abs(out['dtau_e'][n] - per.std() / (np.sqrt(3.0) - 1)) <= 1e-12
    assert out['dtau_e'].min() > 0 and out['dt'] == 2.0
    # one block: no error estimate
    one = noe.finalize_lagged(G[:1], bl[:1], lags, noe.finalize(sums[:1], bl[:1]))
    assert np.all(one['dCdd'] == 0) and np.all(one['dtau_e'] == 0)
    with pytest.raises(ValueError, match='leave a term'):
        noe.finalize_lagged(G, bl, [0, 1, 5, 20], fin)
    with pytest.raises(ValueError, match=r'\(blocks, lags, pairs\)'):
        noe.finalize_lagged(G[:, :3], bl, lags, fin)


def test_write_read_map_ct_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    bl, lags = [30, 30], [1, 2, 4, 9]
    P = 4
    sums, fin, G = _hand_map(rng, bl, lags, P)
    idx = np.array([3, 7, 8, 12])
    res = dict(fin, pairs=noe.pair_list(P), index=idx)
    res.update(noe.finalize_lagged(G, bl, lags, fin, dt=10.0))
    fn = str(tmp_path / 'o_noeMapCt.dat')
    names = ['H%d' % a for a in idx]
    assert noe.write_map_ct(fn, res, names=names) == noe.n_pairs(P)
    with open(fn) as fp:
        head, second = fp.readline(), fp.readline()
    assert head == '# i j name_i name_j tau_e dtau_e Cdd(10) Cdd(20) Cdd(40) Cdd(90)\n' and second == '# lags 10 20 40 90\n'
    tab = noe.read_map_ct(fn)
    pr = res['pairs']
    assert np.array_equal(tab['i'], idx[pr[:, 0]]) and np.array_equal(tab['j'], idx[pr[:, 1]])
    assert tab['name_i'] == [names[i] for i in pr[:, 0]] and tab['name_j'] == [names[j] for j in pr[:, 1]]
    assert np.array_equal(tab['lags'], [10.0, 20.0, 40.0, 90.0])
    for key in ('tau_e', 'dtau_e'):
        assert np.max(np.abs(tab[key] - res[key])) <= 5e-8 * np.max(np.abs(res[key])), key            # %.8g
    assert tab['Cdd'].shape == (noe.n_pairs(P), 4) and np.max(np.abs(tab['Cdd'] - res['Cdd'].T)) <= 5e-8 * np.max(np.abs(res['Cdd']))
    # the cutoff works as in write_map: on reff6
    cut = np.sort(res['reff6'])[2]
    assert noe.write_map_ct(fn, res, cutoff=cut) == 3
    tab = noe.read_map_ct(fn)
    keep = np.nonzero(res['reff6'] <= cut)[0]
    assert np.array_equal(tab['i'], idx[pr[keep, 0]]) and tab['name_j'] == [str(idx[j]) for j in pr[keep, 1]]
    with pytest.raises(ValueError, match='white space'):
        noe.write_map_ct(fn, res, names=['a b', 'c', 'd', 'e'])
    with pytest.raises(ValueError, match='map with lags'):
        noe.write_map_ct(fn, dict(fin, pairs=pr, index=idx))


def test_tau_e_map_floor_and_refusal():
    """tau_e='map' hands the library max(map['tau_e'], TAU_E_FLOOR): zeros (rigid pairs) and values below 1 ps become 1 ps, the others
    pass unchanged; a map without tau_e is a ValueError before anything asks for a GPU"""
    assert noesy.TAU_E_FLOOR == 1e-12
    m = dict(A6=np.ones(6), S2=np.full(6, 0.8), index=np.arange(4), tau_e=np.array([0.0, 3e-13, 1e-12, 2.5e-11, 1e-9, 0.0]))
    got = noesy.map_tau_e(m)
    assert got.dtype == np.float64 and got.tolist() == [1e-12, 1e-12, 1e-12, 2.5e-11, 1e-9, 1e-12]
    assert m['tau_e'][0] == 0.0                                   # the map itself is left alone
    plain = dict(A6=np.ones(6), S2=np.full(6, 0.8), index=np.arange(4))
    for call in (lambda: noesy.map_tau_e(plain), lambda: noesy.rate_matrix(plain, 600.0, 5e-9, tau_e='map'),
                 lambda: noesy.noesy(plain, [0.1], 600.0, 5e-9, tau_e='map')):
        with pytest.raises(ValueError, match='holds no tau_e'):
            call()
    with pytest.raises(ValueError, match="or 'map'"):
        noesy.rate_matrix(m, 600.0, 5e-9, tau_e='auto')


def test_cli_flag_refusals_without_gpu(tmp_path):
    """Every combination of the --noeLag* flags and --noesyTauEMap that does not fit together ends in the script's '= = = ERROR:'
    message and exit status 1 before any GPU work: the input file does not even exist."""
    script = os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')
    base = [sys.executable, script, '-s', 'none.pdb', '-f', str(tmp_path / 'missing.npz'), '-o', str(tmp_path / 'o')]
    full = ['--noeMap', '--noesy', '--noesyMix', '0.05 0.1', '--noesyField', '600', '--noesyTauC', '5e-9']
    cases = [(['--noeLags', '1 2 4'], '--noeLags belongs to --noeMap'),
             (['--noeLagMax', '100'], '--noeLagMax belongs to --noeMap'),
             (['--noeLagCount', '5'], '--noeLagCount belongs to --noeMap'),
             (['--noeMap', '--noeLags', '1 2', '--noeLagMax', '100'], 'give one of them'),
             (['--noeMap', '--noeLagCount', '5'], '--noeLagCount belongs to --noeLagMax'),
             (['--noeMap', '--noeLagMax', '0'], '--noeLagMax must be >= 1'),
             (['--noeMap', '--noeLagMax', '100', '--noeLagCount', '1'], '--noeLagCount 2 .. 64'),
             (['--noeMap', '--noeLagMax', '100', '--noeLagCount', '65'], '--noeLagCount 2 .. 64'),
             (['--noeMap', '--noeLags', ''], '--noeLags must list'),
             (['--noeMap', '--noeLags', '1 2.5'], '--noeLags must list'),
             (['--noeMap', '--noeLags', '1 x'], '--noeLags must list'),
             (['--noeMap', '--noeLags', '2 2'], '--noeLags must list'),
             (['--noeMap', '--noeLags', '4 2'], '--noeLags must list'),
             (['--noeMap', '--noeLags', '-1 2'], '--noeLags must list'),
             (['--noeMap', '--noeLags', ' '.join(str(k) for k in range(65))], '--noeLags must list'),
             (['--noeMap', '--noeLags', '1 2', '--noesyTauEMap'], '--noesyTauEMap belongs to --noesy'),
             (full + ['--noesyTauEMap'], '--noesyTauEMap takes tau_e from the lagged map'),
             (full + ['--noeLags', '1 2', '--noesyTauEMap', '--noesyTauE', '1e-10'], 'both give tau_e'),
             (full + ['--noeLagMax', '16', '--noesyTauEMap', '--noesyTauE', '1e-10'], 'both give tau_e')]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for extra, msg in cases:
        p = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
        err = p.stderr.decode()
        assert p.returncode == 1 and ('= = = ERROR: ' in err) and msg in err, (extra, p.returncode, err[-500:])
        assert not os.listdir(str(tmp_path))


def test_signatures_present():
    _built()
    from ctypes import c_int, c_int64, c_void_p
    from spinrelax_amd import _lib
    names = ('sr_noe_lagged_f32_dev', 'sr_noe_lagged_f32', 'sr_noe_lagged_check', 'sr_noe_lagged_splits')
    for n in names:
        assert n in _lib.SIGNATURES, n
    lib = _lib.load()
    for n in names:
        assert getattr(lib, n).argtypes == _lib.SIGNATURES[n][1]
    assert _lib.SIGNATURES['sr_noe_lagged_f32'][1] == [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int,
                                                       c_void_p, c_int, c_int, c_void_p]
    assert _lib.ABI_VERSION == 13 and lib.sr_abi_version() == 13
    # the split count is host arithmetic: the map's rule, whatever the lags
    assert lib.sr_noe_lagged_splits(5, 300, 1) == 2 and lib.sr_noe_lagged_splits(5, 120, 1) == 1 and lib.sr_noe_lagged_splits(5, 300, 3) == 2
    assert lib.sr_noe_lagged_splits(512, 100000, 1) == 31 and lib.sr_noe_lagged_splits(3000, 100000, 1) == 1
    assert lib.sr_noe_lagged_splits(1, 300, 1) == 0


def test_device_functions_raise_without_gpu():
    """no CPU fallback: on a machine without a GPU the lagged map raises SpinRelaxHipError"""
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    _built()
    from spinrelax_amd._lib import SpinRelaxHipError
    xyz = np.random.default_rng(0).uniform(0, 3, (40, 4, 3)).astype(np.float32)
    with pytest.raises(SpinRelaxHipError):
        noe.dipolar_map(xyz, np.arange(4), lags=[1, 2, 4])
