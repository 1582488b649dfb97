"""
GPU tests (marker gpu) of the time-lagged P2 cross-correlation between pairs of vectors: k_ct_cross (csrc/sr_ct_cross.hip) through
hip.ResidentVectors.ct_cross, spinrelax_amd.ct.calculate_Ct_cross* and the --crossCt flag of scripts/calculate-Ct-from-traj.py.

The oracle is the definition in float64 numpy (oracle_cross below).  Bars:
  * mode 1 (float64 throughout): 1e-12 absolute on C, dC and P0 -- a float64 sum of at most 1000 terms in [0, 1] taken in another
    order differs by about 1e-13;
  * mode 0 (float32 dot products): the bar of the float32 direct-kernel size cases of tests/test_gpu_parity.py
    (test_ct_ragged_and_edge_sizes), quoted: relerr(Ct, Cr) < RTOL = 1e-6 and dct_close(dCt, dCr, R, F), i.e.
    |dCt - dCr| <= max(1e-6 |dCr|, 1e-6 / sqrt(F / 2) / (sqrt(R) - 1)).
The C(t) bar is RELATIVE and a P2 cross-correlation of two arbitrary vectors crosses zero, where a relative error says nothing; the
test vectors wobble by about 0.15 rad around axes that lie within 15 degrees of z, so every pair's C stays above 0.4.
"""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT, relerr
from spinrelax_amd import ct as hostct
from spinrelax_amd import general_scripts as gs
from spinrelax_amd import synth
from spinrelax_amd.hip import SpinRelaxHipError

pytestmark = pytest.mark.gpu

V = 7
RTOL = 1e-6
PAIRS = np.array([(0, 0), (1, 5), (5, 1), (6, 2), (1, 5)], dtype=np.int32)
SIZES = [(F, R) for F in (2, 3, 17, 128, 257, 1000) for R in (1, 3)]


def dct_close(dCt, ref, R, F):
    """tests/test_gpu_parity.py::dct_close"""
    atol = 1e-6 / np.sqrt(F / 2.0) / (np.sqrt(R) - 1.0)
    return np.all(np.abs(dCt - ref) <= np.maximum(RTOL * np.abs(ref), atol))


def make_vectors(N, seed, nV=V):
    """unit vectors (N, nV, 3) float32: an AR(1) wobble of about 0.15 rad around axes within 15 degrees of z"""
    rng = np.random.default_rng(seed)
    tilt, az = np.radians(15.0) * rng.random(nV), 2 * np.pi * rng.random(nV)
    axis = np.stack((np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)), axis=-1)
    e1 = np.cross(axis, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1, axis=-1, keepdims=True)
    e2 = np.cross(axis, e1)
    w = np.empty((N, nV, 2))
    x = 0.15 * rng.standard_normal((nV, 2))
    for t in range(N):
        x = 0.95 * x + 0.15 * np.sqrt(1 - 0.95 ** 2) * rng.standard_normal((nV, 2))
        w[t] = x
    u = axis[None] + w[..., :1] * e1[None] + w[..., 1:] * e2[None]
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    u = u.astype(np.float32)
    return u / np.linalg.norm(u, axis=-1, keepdims=True).astype(np.float32)


def oracle_cross(v4, pairs, sym, lags=None):
    """The definition, float64: v4 (R, F, V, 3) -> P0 (nP), C and dC (L, nP) (or the rows of `lags`)"""
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


@pytest.fixture(scope='module')
def ctx():
    from spinrelax_amd.hip import Context
    c = Context(0)
    yield c
    c.close()


_cache = {}


def case(F, R):
    """vectors of one size case and their oracle for sym = 0 and 1, computed once"""
    if (F, R) not in _cache:
        v4 = make_vectors(R * F, seed=1000 + 10 * F + R).reshape(R, F, V, 3)
        _cache[(F, R)] = (v4, {s: oracle_cross(v4, PAIRS, s) for s in (0, 1)})
    return _cache[(F, R)]


@pytest.mark.parametrize('F,R', SIZES)
def test_float64_mode_against_the_definition(ctx, F, R):
    v4, ref = case(F, R)
    Cp, dCp = hostct.calculate_Ct_Palmer(v4, ctx=ctx, mode=1) if R == 1 else (None, None)
    for sym in (0, 1):
        P0, C, dC = hostct.calculate_Ct_cross(v4, PAIRS, symmetric=bool(sym), ctx=ctx, mode=1)
        P0r, Cr, dCr = ref[sym]
        assert C.shape == dC.shape == (F // 2, len(PAIRS)) and P0.shape == (len(PAIRS),)
        print('F=%d R=%d sym=%d: |dP0| %.2e |dC| %.2e' % (F, R, sym, np.max(np.abs(P0 - P0r)), np.max(np.abs(C - Cr))))
        assert np.max(np.abs(P0 - P0r)) <= 1e-12 and np.max(np.abs(C - Cr)) <= 1e-12
        if R == 1:
            # the reference's std / (sqrt(R) - 1) at R = 1, whatever it gives: the same as C(t)'s own
            np.testing.assert_array_equal(dC, dCp[:, PAIRS[:, 0]])
        else:
            assert np.max(np.abs(dC - dCr)) <= 1e-12
        # a repeated pair and a repeated run give the same bits
        assert C[:, 1].tobytes() == C[:, 4].tobytes() and dC[:, 1].tobytes() == dC[:, 4].tobytes()
    P0b, Cb, dCb = hostct.calculate_Ct_cross(v4, PAIRS, symmetric=True, ctx=ctx, mode=1)
    assert Cb.tobytes() == C.tobytes() and P0b.tobytes() == P0.tobytes()


@pytest.mark.parametrize('F,R', SIZES)
def test_float32_mode_against_the_definition(ctx, F, R):
    v4, ref = case(F, R)
    for sym in (0, 1):
        P0, C, dC = hostct.calculate_Ct_cross(v4, PAIRS, symmetric=bool(sym), ctx=ctx, mode=0)
        P0r, Cr, dCr = ref[sym]
        print('F=%d R=%d sym=%d: relerr P0 %.2e C %.2e' % (F, R, sym, relerr(P0, P0r), relerr(C, Cr)))
        assert relerr(C, Cr) < RTOL and relerr(P0, P0r) < RTOL
        if R == 1:
            assert np.all(np.isnan(dC)) and np.all(np.isnan(dCr))
        else:
            assert dct_close(dC, dCr, R, F)
        assert C[:, 1].tobytes() == C[:, 4].tobytes()               # the repeated pair: the same bits


@pytest.mark.parametrize('F,R', [(257, 3), (1000, 3)])
def test_autocorrelation_identity(ctx, F, R):
    v4, _ = case(F, R)
    diag = np.stack((np.arange(V), np.arange(V)), axis=1)
    for mode in (0, 1):
        Cp, dCp = hostct.calculate_Ct_Palmer(v4, ctx=ctx, mode=mode)
        for sym in (0, 1):
            P0, C, dC = hostct.calculate_Ct_cross(v4, diag, symmetric=bool(sym), ctx=ctx, mode=mode)
            if mode == 1:
                assert np.max(np.abs(C - Cp)) <= 1e-12 and np.max(np.abs(dC - dCp)) <= 1e-12 and np.max(np.abs(P0 - 1.0)) <= 1e-6
            else:
                assert relerr(C, Cp) < RTOL and dct_close(dC, dCp, R, F) and relerr(P0, np.ones(V)) < RTOL


def test_P0_error_over_chunks(ctx):
    """dP0 = std over the chunks of the equal-time value / (sqrt(R) - 1), the formula of dC, from the sums the kernel itself wrote"""
    F, R = 257, 3
    v4, ref = case(F, R)
    a, b = v4[:, :, PAIRS[:, 0]].astype(np.float64), v4[:, :, PAIRS[:, 1]].astype(np.float64)
    per = (1.5 * np.einsum('rtnc,rtnc->rtn', a, b) ** 2 - 0.5).mean(axis=1)
    want = np.std(per, axis=0) / (np.sqrt(R) - 1.0)
    with ctx.vectors(V, R * F) as rv:
        rv.append(v4.reshape(R * F, V, 3))
        for mode in (0, 1):
            P0, dP0, C, dC = hostct.calculate_Ct_cross_resident(rv, PAIRS, R, F, mode=mode, want_dP0=True)
            P0b, Cb, dCb = hostct.calculate_Ct_cross_resident(rv, PAIRS, R, F, mode=mode)
            assert P0.tobytes() == P0b.tobytes() and C.tobytes() == Cb.tobytes() and dC.tobytes() == dCb.tobytes()
            if mode == 1:
                assert np.max(np.abs(dP0 - want)) <= 1e-12
            else:
                assert dct_close(dP0, want, R, 2 * F)          # lag 0 has F terms where dct_close counts F / 2


def test_direction_known_answer(ctx):
    """u_j(t) = u_i(t - 3) inside every chunk: u_i(t) . u_j(t + 3) = 1, so C_ij(3) = 1 while C_ji(3) = <P2(u_i(t) . u_i(t + 6))> < 1.
    A swapped i / j or a lag of the wrong sign exchanges the two."""
    R, F = 3, 200
    s = make_vectors(R * (F + 3), seed=77, nV=1).reshape(R, F + 3, 3)
    v4 = np.ascontiguousarray(np.stack((s[:, 3:], s[:, :F]), axis=2))       # vector 0 = i, vector 1 = j
    pairs = np.array([(0, 1), (1, 0)], dtype=np.int32)
    _, Ca, _ = hostct.calculate_Ct_cross(v4, pairs, symmetric=False, ctx=ctx)
    _, Cs, _ = hostct.calculate_Ct_cross(v4, pairs, symmetric=True, ctx=ctx)
    print('C_ij(3) = %.9f, C_ji(3) = %.6f, symmetric %.6f' % (Ca[2, 0], Ca[2, 1], Cs[2, 0]))
    assert relerr(Ca[2, 0], 1.0) < RTOL
    assert Ca[2, 1] < 0.99
    assert relerr(Cs[2], np.full(2, 0.5 * (Ca[2, 0] + Ca[2, 1]))) < RTOL
    ref = oracle_cross(v4, pairs, 0)[1]
    assert relerr(Ca, ref) < RTOL


def test_rigid_pair(ctx):
    """two constant vectors at an angle theta: C(k) = P0 = P2(cos theta) at every lag, no spread between the chunks"""
    R, F, theta = 3, 300, np.radians(40.0)
    v4 = np.zeros((R, F, 2, 3), dtype=np.float32)
    v4[:, :, 0, 2] = 1.0
    v4[:, :, 1, 0], v4[:, :, 1, 2] = np.sin(theta), np.cos(theta)
    p2 = 1.5 * np.cos(theta) ** 2 - 0.5
    exact = 1.5 * float(v4[0, 0, 1, 2]) ** 2 - 0.5                      # of the float32 components the kernel reads
    for mode in (0, 1):
        for sym in (0, 1):
            P0, C, dC = hostct.calculate_Ct_cross(v4, [(0, 1)], symmetric=bool(sym), ctx=ctx, mode=mode)
            assert abs(P0[0] - p2) < 1e-6 and np.max(np.abs(C - p2)) < 1e-6
            if mode == 1:
                assert abs(P0[0] - exact) <= 1e-12 and np.max(np.abs(C - exact)) <= 1e-12 and np.max(np.abs(dC)) <= 1e-12
            else:
                assert relerr(P0, [exact]) < RTOL and relerr(C, np.full(C.shape, exact)) < RTOL and dct_close(dC, np.zeros(C.shape), R, F)


def test_chunk_table_of_two_files(ctx):
    """per-file tails are dropped exactly as for C(t): the result is that of the whole chunks alone"""
    F = 130
    a, b = make_vectors(3 * F + 41, seed=5), make_vectors(2 * F + 7, seed=6)
    v4 = np.concatenate((a[:3 * F], b[:2 * F])).reshape(5, F, V, 3)
    for sym in (0, 1):
        got = hostct.calculate_Ct_cross_from_files([a, b], 1.0, float(F), PAIRS, symmetric=bool(sym), ctx=ctx)
        want = hostct.calculate_Ct_cross(v4, PAIRS, symmetric=bool(sym), ctx=ctx)
        ref = oracle_cross(v4, PAIRS, sym)
        for g, w, r in zip(got, want, ref):
            assert g.tobytes() == w.tobytes()
        assert relerr(got[0], ref[0]) < RTOL and relerr(got[1], ref[1]) < RTOL and dct_close(got[2], ref[2], 5, F)


def test_capacity(ctx):
    """the longest chunk whose two series fit the LDS, at five probed lags; one frame more is refused before anything runs"""
    F = ctx.ct_cross_max_frames()
    assert F == 6624                                                       # 24 bytes per frame and the padding, in 160 KiB
    L = F // 2
    lags = [1, 2, L // 2, L - 1, L]
    v = make_vectors(F + 1, seed=9, nV=2)
    pairs = np.array([(0, 1)], dtype=np.int32)
    ref = oracle_cross(v[:F].reshape(1, F, 2, 3), pairs, 1, lags=lags)
    with ctx.vectors(2, F + 1) as rv:
        rv.append(v)
        for mode in (0, 1):
            P0, C, dC = hostct.calculate_Ct_cross_resident(rv, pairs, 1, F, mode=mode)
            got = C[np.array(lags) - 1]
            print('mode %d: |dC| at the probed lags %s' % (mode, np.abs(got - ref[1]).ravel()))
            if mode == 1:
                assert np.max(np.abs(got - ref[1])) <= 1e-12 and abs(P0[0] - ref[0][0]) <= 1e-12
            else:
                assert relerr(got, ref[1]) < RTOL and relerr(P0, ref[0]) < RTOL
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_cross(1, F + 1, pairs)
        assert '(-4)' in str(exc.value)
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_cross(1, 100, np.array([(0, 2)], dtype=np.int32))         # an index outside the vectors held
        assert '(-3)' in str(exc.value)


def test_too_many_pairs_are_refused_by_the_check(ctx):
    """one pair more than k_ct_finalize's grid takes (16 x 65535): refused with the other shapes, before anything is queued"""
    pairs = np.zeros((16 * 65535 + 1, 2), dtype=np.int32)
    with ctx.vectors(1, 2) as rv:
        rv.append(make_vectors(2, seed=3, nV=1))
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_cross(1, 2, pairs)
        assert '(-3)' in str(exc.value) and 'too many pairs' in str(exc.value)


def test_the_staged_form_names_the_blocked_one(ctx):
    """one frame beyond the staged limit: the refusal states the limit and where longer chunks go"""
    pairs = np.array([(0, 1)], dtype=np.int32)
    with ctx.vectors(2, 6625) as rv:
        rv.append(make_vectors(6625, seed=9, nV=2))
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_cross(1, 6625, pairs)
        text = str(exc.value)
        assert '(-4)' in text and '6624' in text and 'sr_ct_cross_long_f32_dev' in text and 'no blocked form' not in text


def run(script, *args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', script)] + [str(a) for a in args], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-3000:]


def check_cross_files(d, v4, pr, sym, dt, tau):
    """<d>/o_crossCtint.dat and <d>/o_crossPairs.dat against the definition (the text keeps 8 digits)"""
    R = v4.shape[0]
    P0r, Cr, dCr = oracle_cross(v4, pr, sym)
    legs, t, C, dC = gs.load_sxydylist(str(d / 'o_crossCtint.dat'), 'legend')
    assert [int(x) for x in legs] == list(range(1, len(pr) + 1))
    assert np.allclose(np.array(t)[0], hostct.calculate_dt(dt, tau))
    assert np.max(np.abs(np.array(C) - Cr.T)) < 1e-7 and np.max(np.abs(np.array(dC) - dCr.T)) < 1e-7
    tab = np.loadtxt(str(d / 'o_crossPairs.dat'))
    assert tab.shape == (len(pr), 7)
    assert np.array_equal(tab[:, 0], np.arange(1, len(pr) + 1)) and np.array_equal(tab[:, 1:3], pr)
    assert np.array_equal(tab[:, 3:5], pr + 2)                            # residue ids 2 .. V + 1
    a, b = v4[:, :, pr[:, 0]].astype(np.float64), v4[:, :, pr[:, 1]].astype(np.float64)
    per = (1.5 * np.einsum('rtnc,rtnc->rtn', a, b) ** 2 - 0.5).mean(axis=1)
    assert np.max(np.abs(tab[:, 5] - P0r)) < 1e-7
    assert np.max(np.abs(tab[:, 6] - np.std(per, axis=0) / (np.sqrt(R) - 1.0))) < 1e-7


def test_cli_crossCt(tmp_path, synth_cache):
    """--crossCt --pairs writes its two files, on .npy input too and with --asym; calculate-fitted-Ct.py reads the first; the other
    outputs keep the bytes the existing CLI tests pin (tests/golden/cfg1_*, the run of
    test_gpu_cli.py::test_calculate_Ct_from_traj_dropin), with and without the flag"""
    s = synth.config_shapes(1)
    vecs = synth_cache(1)
    fn = str(tmp_path / 'vecs.npz')
    np.savez(fn, vecs=vecs, names=np.arange(2, 34), dt=s['dt'])
    pf = str(tmp_path / 'pairs.txt')
    with open(pf, 'w') as fp:
        fp.write('# i j\n0 1\n\n3 3   # a diagonal pair\n30 2\n')
    pairs = np.array([(0, 1), (3, 3), (30, 2)])
    q = ' '.join('%.6f' % x for x in synth.Q_EXT)
    common = ['-s', 'reference.pdb', '-f', fn, '--tau', s['tau_memory'], '--vecRot', q, '--vecHist', '--binary', '--vecAvg', '--S2', '--Ct']
    for name, extra in (('plain', []), ('cross', ['--crossCt', '--pairs', pf])):
        (tmp_path / name).mkdir()
        run('calculate-Ct-from-traj.py', *(common + ['-o', str(tmp_path / name / 'o')] + extra))
    new = ['o_crossCtint.dat', 'o_crossPairs.dat']
    plain = sorted(os.listdir(str(tmp_path / 'plain')))
    assert len(plain) >= 5 and sorted(plain + new) == sorted(os.listdir(str(tmp_path / 'cross')))
    for d in ('plain', 'cross'):
        for mine, pinned in (('o_Ctint.dat', 'cfg1_Ctint_f64.dat'), ('o_Ctext.dat', 'cfg1_Ctint_f64.dat'), ('o_avgvec.dat', 'cfg1_avgvec.dat'),
                             ('o_S2.dat', 'cfg1_S2.dat')):
            assert filecmp.cmp(str(tmp_path / d / mine), os.path.join(GOLD, pinned), shallow=False), (d, mine)
    F, R = s['F'], s['R']
    check_cross_files(tmp_path / 'cross', vecs[:R * F].reshape(R, F, -1, 3), pairs, 1, np.float32(s['dt']), s['tau_memory'])
    run('calculate-fitted-Ct.py', '-f', str(tmp_path / 'cross' / 'o_crossCtint.dat'), '-o', str(tmp_path / 'cross' / 'o'))
    assert os.path.isfile(str(tmp_path / 'cross' / 'o_fittedCt.dat'))
    # a small .npy file with a tail that fills no chunk, C_ij and C_ji apart
    small = make_vectors(3 * 64 + 5, seed=21)
    np.save(str(tmp_path / 'small.npy'), small)
    with open(pf, 'w') as fp:
        fp.write('1 5\n6 2\n')
    (tmp_path / 'asym').mkdir()
    run('calculate-Ct-from-traj.py', '-s', 'none.pdb', '-f', str(tmp_path / 'small.npy'), '--dt', 1, '--tau', 64, '-o', str(tmp_path / 'asym' / 'o'),
        '--crossCt', '--pairs', pf, '--asym')
    assert sorted(os.listdir(str(tmp_path / 'asym'))) == new
    check_cross_files(tmp_path / 'asym', small[:192].reshape(3, 64, V, 3), np.array([(1, 5), (5, 1), (6, 2), (2, 6)]), 0, 1.0, 64.0)
