"""
GPU tests (marker gpu) of the blocked form of the pair cross-correlation functions (csrc/sr_ct_cross_long.hip): chunks longer than the
6624 frames k_ct_cross can stage, through hip.ResidentVectors.ct_cross_long, the dispatch of spinrelax_amd.ct.calculate_Ct_cross* and
scripts/calculate-Ct-from-traj.py --crossCt.

The oracle is the definition as six zero-padded float64 numpy.fft cross-correlations (oracle_cross_fft of
tests/test_ct_cross_long_host.py, which holds it against the lag-by-lag definition to 1e-12).  Bars: the cross kernel's own, quoted
from tests/test_gpu_ct_cross.py --
  * mode 1 (float64 throughout): 1e-12 absolute on C, dC and P0;
  * mode 0: relerr(C) < RTOL = 1e-6, relerr(P0) < 1e-6 and dct_close(dC, dCr, R, F), i.e.
    |dC - dCr| <= max(1e-6 |dCr|, 1e-6 / sqrt(F / 2) / (sqrt(R) - 1)).
The test vectors wobble by about 0.15 rad around axes within 15 degrees of z, so every C stays above 0.4 and a relative bar means
something.  Every mode-0 case prints its measured errors (docs/EXPERIMENTS.md section 21 records them).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr
from spinrelax_amd import ct as hostct
from spinrelax_amd import general_scripts as gs
from spinrelax_amd.hip import SpinRelaxHipError
from test_ct_cross_long_host import make_vectors, oracle_cross_fft

pytestmark = pytest.mark.gpu

V = 4
RTOL = 1e-6
PAIRS = np.array([(0, 0), (1, 2), (2, 1), (3, 1), (1, 2)], dtype=np.int32)
SWEEP = [(6625, 3), (8192, 2), (8193, 3), (12289, 2), (20000, 3)]


def dct_close(dCt, ref, R, F):
    """tests/test_gpu_ct_cross.py::dct_close"""
    atol = 1e-6 / np.sqrt(F / 2.0) / (np.sqrt(R) - 1.0)
    return np.all(np.abs(dCt - ref) <= np.maximum(RTOL * np.abs(ref), atol))


def report(tag, got, ref, R, F):
    P0, C, dC = got
    P0r, Cr, dCr = ref
    atol = 1e-6 / np.sqrt(F / 2.0) / (np.sqrt(R) - 1.0)
    with np.errstate(invalid='ignore'):
        print('%s F=%d R=%d: relerr P0 %.2e C %.2e   max |dC - dCr| %.2e (bar: max(1e-6 |dCr|, %.2e))'
              % (tag, F, R, relerr(P0, P0r), relerr(C, Cr), np.nanmax(np.abs(dC - dCr)) if R > 1 else np.nan, atol))


def meets_mode0_bars(got, ref, R, F):
    P0, C, dC = got
    P0r, Cr, dCr = ref
    assert C.shape == dC.shape == (F // 2, len(Cr[0])) and P0.shape == P0r.shape
    assert relerr(C, Cr) < RTOL and relerr(P0, P0r) < RTOL
    if R == 1:
        assert np.all(np.isnan(dC))
    else:
        assert dct_close(dC, dCr, R, F)


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
        v4 = make_vectors(R * F, seed=2000 + 10 * F + R, nV=V).reshape(R, F, V, 3)
        _cache[(F, R)] = (v4, {s: oracle_cross_fft(v4, PAIRS, s) for s in (0, 1)})
    return _cache[(F, R)]


@pytest.mark.parametrize('F,R', SWEEP)
def test_length_sweep_default_dispatch(ctx, F, R):
    """6625: the first length k_ct_cross refuses, nb = 2, nd = 1; 8192: nb = 2 exactly, lag L is offset 1, m = 0; 8193: one sample in the
    last block; 12289: nb = 4, nd = 2; 20000: nb = 5, nd = 3"""
    v4, ref = case(F, R)
    for sym in (0, 1):
        got = hostct.calculate_Ct_cross(v4, PAIRS, symmetric=bool(sym), ctx=ctx, mode=0)
        report('sym=%d' % sym, got, ref[sym], R, F)
        meets_mode0_bars(got, ref[sym], R, F)
        assert got[1][:, 1].tobytes() == got[1][:, 4].tobytes() and got[2][:, 1].tobytes() == got[2][:, 4].tobytes()    # the repeated pair


def test_longest_chunk(ctx):
    F, R = 262144, 2
    assert ctx.ct_cross_long_max_frames() == F
    v4 = make_vectors(R * F, seed=31, nV=2).reshape(R, F, 2, 3)
    pairs = np.array([(0, 1)], dtype=np.int32)
    got = hostct.calculate_Ct_cross(v4, pairs, ctx=ctx)
    ref = oracle_cross_fft(v4, pairs, 1)
    report('sym=1', got, ref, R, F)
    meets_mode0_bars(got, ref, R, F)


@pytest.mark.parametrize('F', [6625, 8193])
def test_float64_mode(ctx, F):
    R = 3
    v4, ref = case(F, R)
    for sym in (0, 1):
        P0, C, dC = hostct.calculate_Ct_cross(v4, PAIRS, symmetric=bool(sym), ctx=ctx, mode=1)
        P0r, Cr, dCr = ref[sym]
        print('F=%d sym=%d: |dP0| %.2e |dC| %.2e' % (F, sym, np.max(np.abs(P0 - P0r)), np.max(np.abs(C - Cr))))
        assert np.max(np.abs(P0 - P0r)) <= 1e-12 and np.max(np.abs(C - Cr)) <= 1e-12 and np.max(np.abs(dC - dCr)) <= 1e-12
        assert C[:, 1].tobytes() == C[:, 4].tobytes()


@pytest.mark.parametrize('F', [5462, 6624])
def test_both_kernels_at_one_length(ctx, F):
    """"ct_cross_long_min_frames" = 5462 sends the lengths k_ct_cross can stage to the blocked form too"""
    R = 3
    v4, ref = case(F, R)
    flat = v4.reshape(R * F, V, 3)
    try:
        ctx.set_option('ct_cross_long_min_frames', 5462)
        with ctx.vectors(V, R * F) as rv:
            rv.append(flat)
            for sym in (0, 1):
                blocked = hostct.calculate_Ct_cross_resident(rv, PAIRS, R, F, symmetric=bool(sym))
                assert blocked[1].tobytes() == rv.ct_cross_long(R, F, PAIRS, sym=sym)[1].tobytes()         # the dispatch took the blocked form
                direct = rv.ct_cross(R, F, PAIRS, sym=sym)
                assert blocked[1].tobytes() != direct[1].tobytes()
                report('blocked, sym=%d' % sym, blocked, ref[sym], R, F)
                report('direct,  sym=%d' % sym, direct, ref[sym], R, F)
                report('blocked against direct, sym=%d' % sym, blocked, direct, R, F)
                meets_mode0_bars(blocked, ref[sym], R, F)
                meets_mode0_bars(direct, ref[sym], R, F)
                meets_mode0_bars(blocked, direct, R, F)
    finally:
        ctx.set_option('ct_cross_long_min_frames', 6625)
    with pytest.raises(SpinRelaxHipError):
        ctx.set_option('ct_cross_long_min_frames', 5461)                 # the floor: the shortest chunk the shared kernels are tested at


def test_autocorrelation_identity(ctx):
    """the pair (v, v) against kernel 1 at the same long chunk"""
    F, R = 8193, 3
    v4, _ = case(F, R)
    diag = np.stack((np.arange(V), np.arange(V)), axis=1)
    Cp, dCp = ctx.ct_palmer(np.ascontiguousarray(v4.reshape(R * F, V, 3)), R, F)
    for sym in (0, 1):
        P0, C, dC = hostct.calculate_Ct_cross(v4, diag, symmetric=bool(sym), ctx=ctx)
        print('sym=%d: relerr against ct_palmer %.2e' % (sym, relerr(C, Cp)))
        assert relerr(C, Cp) < 1e-6 and relerr(P0, np.ones(V)) < 1e-6


def test_same_bits_from_run_to_run_and_for_any_tiling(ctx):
    """F = 20000: 1 MB of spectra per (vector, chunk), 0.2 MB of cross-spectra per (pair, chunk).  8 MiB hold all three chunks of one
    pair but not of two (tiles of pairs); 4 MiB hold one chunk of a pair and of a second that shares a vector (tiles of chunks too)."""
    F, R = 20000, 3
    v4, ref = case(F, R)
    first = hostct.calculate_Ct_cross(v4, PAIRS, ctx=ctx)
    again = hostct.calculate_Ct_cross(v4, PAIRS, ctx=ctx)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    try:
        for mb in (8, 4):
            ctx.set_option('ct_long_ws_mb', mb)
            for sym, want in ((1, first), (0, None)):
                got = hostct.calculate_Ct_cross(v4, PAIRS, symmetric=bool(sym), ctx=ctx)
                if want is None:
                    ctx.set_option('ct_long_ws_mb', 256)
                    want = hostct.calculate_Ct_cross(v4, PAIRS, symmetric=bool(sym), ctx=ctx)
                    ctx.set_option('ct_long_ws_mb', mb)
                for a, b in zip(got, want):
                    assert a.tobytes() == b.tobytes(), mb
    finally:
        ctx.set_option('ct_long_ws_mb', 256)


def test_direction_known_answer(ctx):
    """tests/test_gpu_ct_cross.py::test_direction_known_answer at F = 7000: u_j(t) = u_i(t - 3) inside every chunk, so C_ij(3) = 1 while
    C_ji(3) = <P2(u_i(t) . u_i(t + 6))> < 1.  A swapped i / j or a lag of the wrong sign exchanges the two."""
    R, F = 3, 7000
    s = make_vectors(R * (F + 3), seed=77, nV=1).reshape(R, F + 3, 3)
    v4 = np.ascontiguousarray(np.stack((s[:, 3:], s[:, :F]), axis=2))       # vector 0 = i, vector 1 = j
    pairs = np.array([(0, 1), (1, 0)], dtype=np.int32)
    _, Ca, _ = hostct.calculate_Ct_cross(v4, pairs, symmetric=False, ctx=ctx)
    _, Cs, _ = hostct.calculate_Ct_cross(v4, pairs, symmetric=True, ctx=ctx)
    print('C_ij(3) = %.9f, C_ji(3) = %.6f, symmetric %.6f' % (Ca[2, 0], Ca[2, 1], Cs[2, 0]))
    assert relerr(Ca[2, 0], 1.0) < RTOL
    assert Ca[2, 1] < 0.99
    assert relerr(Cs[2], np.full(2, 0.5 * (Ca[2, 0] + Ca[2, 1]))) < RTOL
    assert relerr(Ca, oracle_cross_fft(v4, pairs, 0)[1]) < RTOL


def test_series_kinds(ctx):
    """series that are not unit-vector series take |u|^2 as a sixth signal, and so does the unit series they are paired with: a scaled
    vector, one with a few zero frames, one with a single frame just outside the unit tolerance; pair by pair against the oracle"""
    F, R = 8193, 3
    v4 = case(F, R)[0].copy()
    v4[:, :, 1] *= np.float32(1.7)
    v4[1, 100:103, 2] = 0.0
    v4[2, 5000, 3] *= np.float32(1.0 + 2e-6)
    pairs = np.array([(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 3), (3, 0), (3, 3), (1, 2)], dtype=np.int32)
    for mode in (0, 1):
        for sym in (0, 1):
            got = hostct.calculate_Ct_cross(v4, pairs, symmetric=bool(sym), ctx=ctx, mode=mode)
            ref = oracle_cross_fft(v4, pairs, sym)
            for n in range(len(pairs)):
                g, r = [x[..., n:n + 1] for x in got], [x[..., n:n + 1] for x in ref]
                if mode == 1:
                    assert max(np.max(np.abs(a - b)) for a, b in zip(g, r)) <= 1e-12, (mode, sym, n)
                else:
                    report('pair %d (%d, %d) sym=%d' % (n, pairs[n][0], pairs[n][1], sym), g, r, R, F)
                    assert relerr(g[1], r[1]) < RTOL and relerr(g[0], r[0]) < RTOL, (sym, n)
                    assert dct_close(g[2], r[2], R, F), (sym, n)


def test_rigid_pair_and_a_single_chunk(ctx):
    """two constant vectors at 40 degrees: C(k) = P0 = P2(cos theta) at every lag, no spread between the chunks; R = 1: dC is NaN"""
    F, theta = 8193, np.radians(40.0)
    for R in (3, 1):
        v4 = np.zeros((R, F, 2, 3), dtype=np.float32)
        v4[:, :, 0, 2] = 1.0
        v4[:, :, 1, 0], v4[:, :, 1, 2] = np.sin(theta), np.cos(theta)
        exact = 1.5 * float(v4[0, 0, 1, 2]) ** 2 - 0.5                      # of the float32 components the kernel reads
        for mode in (0, 1):
            for sym in (0, 1):
                P0, C, dC = hostct.calculate_Ct_cross(v4, [(0, 1)], symmetric=bool(sym), ctx=ctx, mode=mode)
                print('R=%d mode %d sym=%d: |P0 - exact| %.2e max |C - exact| %.2e' % (R, mode, sym, abs(P0[0] - exact), np.max(np.abs(C - exact))))
                if R == 1:
                    assert np.all(np.isnan(dC))
                if mode == 1:
                    assert abs(P0[0] - exact) <= 1e-12 and np.max(np.abs(C - exact)) <= 1e-12
                    assert R == 1 or np.max(np.abs(dC)) <= 1e-12
                else:
                    assert relerr(P0, [exact]) < RTOL and relerr(C, np.full(C.shape, exact)) < RTOL
                    assert R == 1 or dct_close(dC, np.zeros(C.shape), R, F)


def test_chunk_table_of_two_files(ctx):
    """odd chunk starts: per-file tails are dropped exactly as for C(t), the result is that of the whole chunks alone"""
    F = 7001
    a, b = make_vectors(2 * F + 41, seed=5, nV=V), make_vectors(F + 7, seed=6, nV=V)
    v4 = np.concatenate((a[:2 * F], b[:F])).reshape(3, F, V, 3)
    for sym in (0, 1):
        got = hostct.calculate_Ct_cross_from_files([a, b], 1.0, float(F), PAIRS, symmetric=bool(sym), ctx=ctx)
        want = hostct.calculate_Ct_cross(v4, PAIRS, symmetric=bool(sym), ctx=ctx)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
        meets_mode0_bars(got, oracle_cross_fft(v4, PAIRS, sym), 3, F)


def test_refusals(ctx):
    pairs = np.array([(0, 1)], dtype=np.int32)
    v = make_vectors(7000, seed=9, nV=2)
    with ctx.vectors(2, 7000) as rv:
        rv.append(v)
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_cross_long(1, 262145, pairs)
        assert '(-4)' in str(exc.value)
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_cross_long(1, 7000, np.array([(0, 2)], dtype=np.int32))    # an index outside the vectors held
        assert '(-3)' in str(exc.value)
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_cross(1, 6625, pairs)                                       # the staged kernel keeps its limit
        assert '(-4)' in str(exc.value)
        with pytest.raises(ValueError) as exc:
            hostct.calculate_Ct_cross_resident(rv, pairs, 1, 262145)
        assert '6624' in str(exc.value) and '262144' in str(exc.value)
        rv.ct_cross_long(1, 7000, pairs)                                       # and the object still works


def test_too_many_pairs_are_refused_by_the_check(ctx):
    """one pair more than k_ct_finalize's grid takes (16 x 65535) at the shortest blocked chunk: refused with the other shapes, before
    the work area for the raw sums of a million pairs is asked for"""
    pairs = np.zeros((16 * 65535 + 1, 2), dtype=np.int32)
    with ctx.vectors(1, 5462) as rv:
        rv.append(make_vectors(5462, seed=3, nV=1))
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_cross_long(1, 5462, pairs)
        assert '(-3)' in str(exc.value) and 'too many pairs' in str(exc.value)


def run(script, *args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', script)] + [str(a) for a in args], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-3000:]


def check_cross_files(d, v4, pr, sym, dt, tau):
    """tests/test_gpu_ct_cross.py::check_cross_files with the FFT oracle: <d>/o_crossCtint.dat and <d>/o_crossPairs.dat (8 digits)"""
    R = v4.shape[0]
    P0r, Cr, dCr = oracle_cross_fft(v4, pr, sym)
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


def test_cli_crossCt_long_tau(tmp_path):
    """--crossCt at a --tau beyond the staged kernel, no new flag; with --asym; calculate-fitted-Ct.py reads the first file"""
    F = 7000
    vecs = make_vectors(2 * F + 5, seed=21, nV=V)
    np.save(str(tmp_path / 'vecs.npy'), vecs)
    pf = str(tmp_path / 'pairs.txt')
    with open(pf, 'w') as fp:
        fp.write('1 2\n3 0\n')
    v4 = vecs[:2 * F].reshape(2, F, V, 3)
    new = ['o_crossCtint.dat', 'o_crossPairs.dat']
    for name, extra, pr, sym in (('sym', [], np.array([(1, 2), (3, 0)]), 1),
                                 ('asym', ['--asym'], np.array([(1, 2), (2, 1), (3, 0), (0, 3)]), 0)):
        (tmp_path / name).mkdir()
        run('calculate-Ct-from-traj.py', '-s', 'none.pdb', '-f', str(tmp_path / 'vecs.npy'), '--dt', 1, '--tau', F, '-o', str(tmp_path / name / 'o'),
            '--crossCt', '--pairs', pf, *extra)
        assert sorted(os.listdir(str(tmp_path / name))) == new
        check_cross_files(tmp_path / name, v4, pr, sym, 1.0, float(F))
    run('calculate-fitted-Ct.py', '-f', str(tmp_path / 'sym' / 'o_crossCtint.dat'), '-o', str(tmp_path / 'sym' / 'o'))
    assert os.path.isfile(str(tmp_path / 'sym' / 'o_fittedCt.dat'))
