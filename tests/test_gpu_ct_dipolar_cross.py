"""
GPU tests (marker gpu) of the distance-weighted P2 cross-correlation between pairs of flexible spin pairs: k_ct_dipolar_cross and
k_ct_dipolar_cross_norm (csrc/sr_ct_dipolar_cross.hip) through Context.ct_dipolar_cross_dev, hip.ResidentVectors.ct_dipolar_cross,
spinrelax_amd.ct.calculate_Ct_dipolar_cross* and the --dipolarCrossCt flag of scripts/calculate-Ct-from-traj.py.

The oracle is the definition in float64 numpy (oracle_core / oracle_dcross below), chunk-pooled like the library: per chunk
c_r(k) = [1.5 sum (a_i . a_j')^2 - 0.5 sum w_i w_j'] / (F - k), k = 0 .. F/2 (symmetric: the mean of both directions), per vector
n_v = mean_r sum w_v^2 / F; C = mean_r c_r / sqrt(n_i n_j), dC = std_r c_r / (sqrt(R) - 1) / sqrt(n_i n_j), P0 and dP0 from k = 0.
Bars, the project's own (tests/test_gpu_ct_cross.py, tests/test_gpu_parity.py):
  * mode 1 (float64 throughout) against the definition on the planes the pack wrote: 1e-12 absolute on C, dC, P0 and dP0;
  * mode 0 (float32 products) against the definition on the raw vectors: relerr < 1e-6 on C and P0, dct_close on dC (and on dP0 with
    2 F in the place of F: lag 0 has F terms where dct_close counts F / 2, as in test_gpu_ct_cross.py); reff6 1e-6 relative.
The relative bar needs C away from zero: the vectors of tests/test_gpu_ct_dipolar.py::make_pairs keep every pair's C and P0 above 0.4
(asserted on the oracle; 0.476 at worst).
"""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr
from test_gpu_ct_cross import dct_close
from test_gpu_ct_dipolar import dev_pack, exact_unit_vectors, make_pairs, planes_of
from spinrelax_amd import ct as hostct
from spinrelax_amd import general_scripts as gs
from spinrelax_amd.hip import SpinRelaxHipError

pytestmark = pytest.mark.gpu

V = 7
RTOL = 1e-6
PAIRS = np.array([(0, 0), (1, 5), (5, 1), (6, 2), (1, 5)], dtype=np.int32)
PAIRS3 = np.array([(0, 0), (1, 2), (2, 1), (0, 2)], dtype=np.int32)
SIZES = [(F, R) for F in (2, 3, 17, 128, 257, 1000) for R in (1, 3)]
# F <= 254: the float64 path alone; 257 and 1000: full lag blocks and a tail of lags behind them, some waves without a block; 4096 and
# 4100: 16 blocks, two per wave, 4100 with three lags behind them
SIZES32 = [(F, R, V) for F, R in SIZES] + [(4096, 2, 3), (4100, 2, 3)]


def pairs_of(nV):
    return PAIRS if nV == V else PAIRS3


def oracle_core(a4, w4, pairs, sym, lags=None):
    """a4 (R, F, V, 3), w4 (R, F, V) -> P0, dP0 (nP), C, dC (L or len(lags), nP) and <w^2> (V) over the chunks: the definition, float64"""
    a4, w4 = np.asarray(a4, dtype=np.float64), np.asarray(w4, dtype=np.float64)
    pairs = np.asarray(pairs)
    R, F = w4.shape[:2]
    ks = np.arange(0, F // 2 + 1) if lags is None else np.concatenate(([0], np.asarray(lags)))
    ai, aj, wi, wj = a4[:, :, pairs[:, 0]], a4[:, :, pairs[:, 1]], w4[:, :, pairs[:, 0]], w4[:, :, pairs[:, 1]]
    c = np.empty((len(ks), R, len(pairs)))
    for m, k in enumerate(ks):
        Sa = (np.einsum('rtpc,rtpc->rtp', ai[:, :F - k], aj[:, k:]) ** 2).sum(axis=1)
        Sw = (wi[:, :F - k] * wj[:, k:]).sum(axis=1)
        if sym:
            Sa = 0.5 * (Sa + (np.einsum('rtpc,rtpc->rtp', aj[:, :F - k], ai[:, k:]) ** 2).sum(axis=1))
            Sw = 0.5 * (Sw + (wj[:, :F - k] * wi[:, k:]).sum(axis=1))
        c[m] = (1.5 * Sa - 0.5 * Sw) / (F - k)
    n = ((w4 ** 2).sum(axis=1) / F).mean(axis=0)
    norm = np.sqrt(n[pairs[:, 0]] * n[pairs[:, 1]])
    with np.errstate(divide='ignore', invalid='ignore'):
        d = np.std(c, axis=1) / (np.sqrt(R) - 1.0) / norm
    m = c.mean(axis=1) / norm
    return m[0], d[0], m[1:], d[1:], (w4 ** 2).mean(axis=(0, 1))


def oracle_dcross(vec, dist, pairs, sym, R, F, starts=None, lags=None):
    """vec (N, V, 3), dist (N, V) or None, chunks of F frames at `starts` (default r F) -> P0, dP0, C, dC, reff6 (nP, 2)"""
    a, w, rref = planes_of(vec, dist)
    starts = np.arange(R) * F if starts is None else starts
    a4 = np.stack([a[s:s + F] for s in starts])
    w4 = np.stack([w[s:s + F] for s in starts])
    P0, dP0, C, dC, w2 = oracle_core(a4, w4, pairs, sym, lags)
    return P0, dP0, C, dC, (rref * w2 ** (-1.0 / 6.0))[np.asarray(pairs)]


@pytest.fixture(scope='module')
def ctx():
    from spinrelax_amd.hip import Context
    c = Context(0)
    yield c
    c.close()


_cache = {}


def case(F, R, nV=V):
    """(u, r, raw) of one size case and the oracle of the raw vectors for sym = 0 and 1, computed once"""
    if (F, R, nV) not in _cache:
        u, r, raw = make_pairs(R * F, seed=6000 + 10 * F + R, nV=nV)
        _cache[(F, R, nV)] = (u, r, raw, {s: oracle_dcross(raw, None, pairs_of(nV), s, R, F) for s in (0, 1)})
    return _cache[(F, R, nV)]


def dev_ct(ctx, planes, Npad, nV, R, F, pairs, sym, mode):
    """sr_ct_dipolar_cross_f32_dev on device planes: P0, dP0, C, dC and wsum2 (nP, R, 2), downloaded"""
    import torch
    L, nP = F // 2, len(pairs)
    P0 = torch.empty((2, nP), device='cuda', dtype=torch.float64)
    Ct = torch.empty((L, nP), device='cuda', dtype=torch.float64)
    dCt = torch.empty((L, nP), device='cuda', dtype=torch.float64)
    ws = torch.empty((nP, R, 2), device='cuda', dtype=torch.float64)
    ctx.ct_dipolar_cross_dev(planes.data_ptr(), Npad, nV, R, F, pairs, P0[0].data_ptr(), Ct.data_ptr(), dCt.data_ptr(), ws.data_ptr(), sym=sym,
                             mode=mode, dP0_ptr=P0[1].data_ptr())
    ctx.sync()
    P0 = P0.cpu().numpy()
    return P0[0], P0[1], Ct.cpu().numpy(), dCt.cpu().numpy(), ws.cpu().numpy()


def close32(got, ref, R, F):
    """the float32 bars on (P0, dP0, C, dC)"""
    P0, dP0, C, dC = got[:4]
    P0r, dP0r, Cr, dCr = ref[:4]
    ok = relerr(C, Cr) < RTOL and relerr(P0, P0r) < RTOL
    if R == 1:
        return ok and np.all(np.isnan(dC)) and np.all(np.isnan(dP0))
    return ok and dct_close(dC, dCr, R, F) and dct_close(dP0, dP0r, R, 2 * F)


@pytest.mark.parametrize('F,R', SIZES)
def test_float64_mode_against_the_definition_on_the_planes(ctx, F, R):
    u, r, raw, _ = case(F, R)
    p, rref, planes, Npad = dev_pack(ctx, raw, None)
    a4 = p[:, :3, :R * F].transpose(2, 0, 1).reshape(R, F, V, 3)
    w4 = p[:, 3, :R * F].T.reshape(R, F, V).astype(np.float64)
    Cp, dCp = hostct.calculate_Ct_Palmer(u.reshape(R, F, V, 3), ctx=ctx, mode=1) if R == 1 else (None, None)
    for sym in (0, 1):
        P0, dP0, C, dC, ws = dev_ct(ctx, planes, Npad, V, R, F, PAIRS, sym, 1)
        P0r, dP0r, Cr, dCr, _ = oracle_core(a4, w4, PAIRS, sym)
        assert C.shape == dC.shape == (F // 2, len(PAIRS)) and P0.shape == (len(PAIRS),)
        w2 = (w4 ** 2).sum(axis=1).T                                       # (V, R)
        print('F=%d R=%d sym=%d: |dP0| %.2e |dC| %.2e wsum2 %.2e' % (F, R, sym, np.max(np.abs(P0 - P0r)), np.max(np.abs(C - Cr)),
                                                                      relerr(ws[:, :, 0], w2[PAIRS[:, 0]])))
        assert np.max(np.abs(P0 - P0r)) <= 1e-12 and np.max(np.abs(C - Cr)) <= 1e-12
        assert relerr(ws[:, :, 0], w2[PAIRS[:, 0]]) <= 1e-12 and relerr(ws[:, :, 1], w2[PAIRS[:, 1]]) <= 1e-12
        if R == 1:
            # the reference's std / (sqrt(R) - 1) at R = 1, whatever it gives: the same as C(t)'s own
            np.testing.assert_array_equal(dC, dCp[:, PAIRS[:, 0]])
        else:
            assert np.max(np.abs(dC - dCr)) <= 1e-12 and np.max(np.abs(dP0 - dP0r)) <= 1e-12
        # a repeated pair and a repeated run give the same bits
        assert C[:, 1].tobytes() == C[:, 4].tobytes() and dC[:, 1].tobytes() == dC[:, 4].tobytes() and P0[1].tobytes() == P0[4].tobytes()
    again = dev_ct(ctx, planes, Npad, V, R, F, PAIRS, 1, 1)
    for g, w in zip((P0, dP0, C, dC, ws), again):
        assert g.tobytes() == w.tobytes()


@pytest.mark.parametrize('F,R,nV', SIZES32)
def test_float32_mode_against_the_definition(ctx, F, R, nV):
    u, r, raw, ref = case(F, R, nV)
    pairs = pairs_of(nV)
    lo = min(min(ref[s][0].min(), ref[s][2].min()) for s in (0, 1))
    assert lo >= 0.4
    for sym in (0, 1):
        got = hostct.calculate_Ct_dipolar_cross(raw.reshape(R, F, nV, 3), pairs, symmetric=bool(sym), ctx=ctx, mode=0)
        P0, dP0, C, dC, reff6 = got
        print('F=%d R=%d sym=%d: min %.3f relerr P0 %.2e C %.2e reff6 %.2e' % (F, R, sym, lo, relerr(P0, ref[sym][0]), relerr(C, ref[sym][2]),
                                                                               relerr(reff6, ref[sym][4])))
        assert C.shape == dC.shape == (F // 2, len(pairs)) and reff6.shape == (len(pairs), 2)
        assert close32(got, ref[sym], R, F)
        assert relerr(reff6, ref[sym][4]) < RTOL
        if nV == V:
            assert C[:, 1].tobytes() == C[:, 4].tobytes()               # the repeated pair: the same bits
        again = hostct.calculate_Ct_dipolar_cross(raw.reshape(R, F, nV, 3), pairs, symmetric=bool(sym), ctx=ctx, mode=0)
        for g, w in zip(got, again):
            assert g.tobytes() == w.tobytes()                              # two runs: the same bytes
    if F == 257:
        # the other input form: unit vectors and the distances beside them
        alt = hostct.calculate_Ct_dipolar_cross(u.reshape(R, F, nV, 3), pairs, dist=r.reshape(R, F, nV), ctx=ctx, mode=0)
        refd = oracle_dcross(u, r, pairs, 1, R, F)
        assert close32(alt, refd, R, F) and relerr(alt[4], refd[4]) < RTOL


@pytest.mark.parametrize('F,R', [(257, 3), (1000, 3)])
def test_diagonal_pairs_are_the_dipolar_autocorrelation(ctx, F, R):
    u, r, raw, _ = case(F, R)
    v4 = raw.reshape(R, F, V, 3)
    diag = np.stack((np.arange(V), np.arange(V)), axis=1)
    for mode in (0, 1):
        Cd, dCd, reff6d = hostct.calculate_Ct_dipolar(v4, ctx=ctx, mode=mode)[:3]
        for sym in (0, 1):
            P0, dP0, C, dC, reff6 = hostct.calculate_Ct_dipolar_cross(v4, diag, symmetric=bool(sym), ctx=ctx, mode=mode)
            print('F=%d mode %d sym %d: |dC| %.2e |P0 - 1| %.2e' % (F, mode, sym, np.max(np.abs(C - Cd)), np.max(np.abs(P0 - 1.0))))
            if mode == 1:
                assert np.max(np.abs(C - Cd)) <= 1e-12 and np.max(np.abs(dC - dCd)) <= 1e-12
            else:
                assert relerr(C, Cd) < RTOL and dct_close(dC, dCd, R, F)
            assert np.max(np.abs(P0 - 1.0)) <= 1e-6
            assert np.array_equal(reff6[:, 0], reff6[:, 1]) and relerr(reff6[:, 0], reff6d) < RTOL


@pytest.mark.parametrize('F,R', [(257, 3), (1000, 3)])
def test_constant_distances_give_the_unit_vector_cross_correlation(ctx, F, R):
    """unit vectors, each at its own constant distance (given beside them): w = 1 and a = u, bit for bit, so the result is C_ij"""
    d = np.linspace(0.2, 0.5, V).astype(np.float32)
    u = exact_unit_vectors(R * F, seed=31 + F)
    v4 = u.reshape(R, F, V, 3)
    dist = np.broadcast_to(d, (R, F, V))
    for mode in (0, 1):
        for sym in (0, 1):
            P0x, Cx, dCx = hostct.calculate_Ct_cross(v4, PAIRS, symmetric=bool(sym), ctx=ctx, mode=mode)
            P0, dP0, C, dC, reff6 = hostct.calculate_Ct_dipolar_cross(v4, PAIRS, dist=dist, symmetric=bool(sym), ctx=ctx, mode=mode)
            if mode == 1:
                assert np.max(np.abs(C - Cx)) <= 1e-12 and np.max(np.abs(dC - dCx)) <= 1e-12 and np.max(np.abs(P0 - P0x)) <= 1e-12
            else:
                assert relerr(C, Cx) < RTOL and relerr(P0, P0x) < RTOL and dct_close(dC, dCx, R, F)
            assert relerr(reff6, d.astype(np.float64)[PAIRS]) <= 1e-7


@pytest.mark.parametrize('p2,axis_j', [(1.0, 2), (-0.5, 0)])
@pytest.mark.parametrize('in_phase', [True, False])
def test_known_answer_alternating_distances(ctx, p2, axis_j, in_phase):
    """Vector i along z, vector j along z (P2 = 1) or x (P2 = -0.5); both distances alternate r, 4 r frame by frame, in phase or out of
    phase: w in {1, 1/64} and sqrt(w) in {1, 1/8} are float32 numbers.  With (w1, w2) the weights of i and (v1, v2) those of j at
    even and odd frames, F even and sym = 1: C(k) = P2 (w1 v1 + w2 v2) / sqrt((w1^2 + w2^2)(v1^2 + v2^2)) for even k (k = 0 too);
    for odd k the cross terms w1 v2 + w2 v1 (both directions together see every frame parity equally often)."""
    R, F, r1, r2 = 3, 200, 0.25, 1.0
    v = np.zeros((R * F, 2, 3), dtype=np.float32)
    v[0::2, 0, 2], v[1::2, 0, 2] = r1, r2
    rj = (r1, r2) if in_phase else (r2, r1)
    v[0::2, 1, axis_j], v[1::2, 1, axis_j] = rj
    w1, w2 = 1.0, (r1 / r2) ** 3
    v1, v2 = (w1, w2) if in_phase else (w2, w1)
    den = np.sqrt((w1 * w1 + w2 * w2) * (v1 * v1 + v2 * v2))
    even, odd = p2 * (w1 * v1 + w2 * v2) / den, p2 * (w1 * v2 + w2 * v1) / den
    want = np.where(np.arange(1, F // 2 + 1) % 2 == 0, even, odd)[:, None]
    for mode in (0, 1):
        P0, dP0, C, dC, reff6 = hostct.calculate_Ct_dipolar_cross(v.reshape(R, F, 2, 3), [(0, 1)], ctx=ctx, mode=mode)
        print('P2 %.1f in phase %d mode %d: |dC| %.2e |dP0| %.2e' % (p2, in_phase, mode, np.max(np.abs(C - want)), abs(P0[0] - even)))
        if mode == 1:
            assert np.max(np.abs(C - want)) <= 1e-12 and abs(P0[0] - even) <= 1e-12 and np.max(np.abs(dC)) <= 1e-12
        else:
            assert relerr(C, want) < RTOL and relerr(P0, [even]) < RTOL
        assert relerr(reff6, np.full((1, 2), r1 * (0.5 * (w1 * w1 + w2 * w2)) ** (-1.0 / 6.0))) < RTOL


def test_asymmetric_directions_average_to_the_symmetric_function(ctx):
    F, R = 257, 3
    u, r, raw, _ = case(F, R)
    v4 = raw.reshape(R, F, V, 3)
    Pa, _, Ca, _, _ = hostct.calculate_Ct_dipolar_cross(v4, PAIRS, symmetric=False, ctx=ctx, mode=1)
    Pb, _, Cb, _, _ = hostct.calculate_Ct_dipolar_cross(v4, PAIRS[:, ::-1], symmetric=False, ctx=ctx, mode=1)
    Ps, _, Cs, _, _ = hostct.calculate_Ct_dipolar_cross(v4, PAIRS, symmetric=True, ctx=ctx, mode=1)
    assert np.max(np.abs(0.5 * (Ca + Cb) - Cs)) <= 1e-12 and np.max(np.abs(0.5 * (Pa + Pb) - Ps)) <= 1e-12
    assert np.max(np.abs(Ca[:, 1] - Cb[:, 1])) > 1e-6                      # the two directions do differ


def test_ragged_chunks(ctx):
    """the chunk table of test_gpu_ct_dipolar.py::test_ragged_chunks against the oracle on the same windows; the other analyses of the
    same object return the same bytes before and after"""
    F = 130
    u, r, raw = make_pairs(5 * F + 48 + 7, seed=5)
    starts = np.array([0, F + 3, 2 * F + 3, 3 * F + 41, 4 * F + 48], dtype=np.int64)
    with ctx.vectors(V, raw.shape[0]) as rv:
        rv.append(raw)
        before = rv.ct(5, F, chunk_start=starts) + rv.ct_dipolar(5, F, chunk_start=starts) + rv.ct_cross(5, F, PAIRS, chunk_start=starts)
        for mode in (0, 1):
            for sym in (0, 1):
                got = hostct.calculate_Ct_dipolar_cross_resident(rv, PAIRS, 5, F, symmetric=bool(sym), mode=mode, chunk_start=starts)
                ref = oracle_dcross(raw, None, PAIRS, sym, 5, F, starts=starts)
                assert close32(got, ref, 5, F) and relerr(got[4], ref[4]) < RTOL
        after = rv.ct(5, F, chunk_start=starts) + rv.ct_dipolar(5, F, chunk_start=starts) + rv.ct_cross(5, F, PAIRS, chunk_start=starts)
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes()
        bad = starts.copy()
        bad[4] = raw.shape[0] - F + 1
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_dipolar_cross(5, F, PAIRS, chunk_start=bad)
        assert '(-3)' in str(exc.value)


def test_limits(ctx):
    """the longest chunk whose eight series fit the LDS, at 16 probed lags; one frame more is refused before anything runs; so are a
    pair outside the vectors and a vector without a direction"""
    F = ctx.ct_dipolar_cross_max_frames()
    assert F == 4896                                                       # 32 bytes per frame and the padding, in 160 KiB
    L = F // 2
    lags = np.unique(np.linspace(1, L, 16).astype(int))
    assert len(lags) == 16
    u, r, raw = make_pairs(F + 1, seed=9, nV=2)
    pairs = np.array([(0, 1)], dtype=np.int32)
    ref = oracle_dcross(raw, None, pairs, 1, 1, F, lags=lags)
    assert min(ref[0].min(), ref[2].min()) >= 0.4
    with ctx.vectors(2, F + 1) as rv:
        rv.append(raw)
        P0, dP0, C, dC, reff6 = hostct.calculate_Ct_dipolar_cross_resident(rv, pairs, 1, F, mode=0)
        print('F=%d: relerr at the probed lags %.2e P0 %.2e' % (F, relerr(C[lags - 1], ref[2]), relerr(P0, ref[0])))
        assert relerr(C[lags - 1], ref[2]) < RTOL and relerr(P0, ref[0]) < RTOL and relerr(reff6, ref[4]) < RTOL
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_dipolar_cross(1, F + 1, pairs)
        assert '(-4)' in str(exc.value) and '4896' in str(exc.value)
        with pytest.raises(ValueError):
            hostct.calculate_Ct_dipolar_cross_resident(rv, [(0, 2)], 1, 100)
    raw[40, 1] = 0.0
    with ctx.vectors(2, F + 1) as rv:
        rv.append(raw)
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_dipolar_cross(1, 100, pairs)
        assert '(-3)' in str(exc.value) and 'vector 1' in str(exc.value)


def run(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')] + [str(a) for a in args],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)


def check_files(d, want, pairs, names, dt, tau):
    """<d>/o_dipolarCrossCtint.dat and <d>/o_dipolarCrossPairs.dat against the API's arrays (the text keeps 8 digits)"""
    P0, dP0, C, dC, reff6 = want
    legs, t, Cf, dCf = gs.load_sxydylist(str(d / 'o_dipolarCrossCtint.dat'), 'legend')
    assert [int(x) for x in legs] == list(range(1, len(pairs) + 1))
    assert np.allclose(np.array(t)[0], hostct.calculate_dt(dt, tau))
    assert np.max(np.abs(np.array(Cf) - C.T)) < 1e-7 and np.max(np.abs(np.array(dCf) - dC.T)) < 1e-7
    with open(str(d / 'o_dipolarCrossPairs.dat')) as fp:
        assert fp.readline().rstrip('\n') == '# pair i j resid_i resid_j P0 dP0 reff6_i reff6_j'
    tab = np.loadtxt(str(d / 'o_dipolarCrossPairs.dat'), ndmin=2)
    assert tab.shape == (len(pairs), 9)
    assert np.array_equal(tab[:, 0], np.arange(1, len(pairs) + 1)) and np.array_equal(tab[:, 1:3], pairs)
    assert np.array_equal(tab[:, 3:5], np.asarray(names)[pairs])
    assert np.max(np.abs(tab[:, 5] - P0)) < 1e-7 and np.max(np.abs(tab[:, 6] - dP0)) < 1e-7
    assert relerr(tab[:, 7:9], reff6) < 1e-7


def test_cli_dipolarCrossCt(tmp_path, ctx):
    """--dipolarCrossCt --pairs on an .npz with vecs + dist, with and without --asym, writes its two files, which agree with the API;
    the files of --Ct --crossCt --dipolarCt beside it are the bytes they are without it; without --pairs the parser refuses"""
    F, R = 64, 3
    u, r, raw = make_pairs(R * F + 5, seed=21)
    names = np.arange(11, 11 + V)
    fn = str(tmp_path / 'pairs.npz')
    np.savez(fn, vecs=u, dist=r, names=names, dt=1.0)
    pf = str(tmp_path / 'pairs.txt')
    with open(pf, 'w') as fp:
        fp.write('# i j\n1 5\n3 3\n6 2\n')
    pairs = np.array([(1, 5), (3, 3), (6, 2)])
    common = ['-s', 'none.pdb', '-f', fn, '--tau', F, '--Ct', '--crossCt', '--dipolarCt', '--pairs', pf]
    new = ['o_dipolarCrossCtint.dat', 'o_dipolarCrossPairs.dat']
    for name, extra in (('plain', []), ('new', ['--dipolarCrossCt']), ('asym', ['--dipolarCrossCt', '--asym']), ('plain_asym', ['--asym'])):
        (tmp_path / name).mkdir()
        p = run(*(common + ['-o', str(tmp_path / name / 'o')] + extra))
        assert p.returncode == 0, p.stdout.decode()[-3000:]
    for a, b in (('plain', 'new'), ('plain_asym', 'asym')):
        old = sorted(os.listdir(str(tmp_path / a)))
        assert len(old) == 6 and sorted(old + new) == sorted(os.listdir(str(tmp_path / b)))
        for f in old:
            assert filecmp.cmp(str(tmp_path / a / f), str(tmp_path / b / f), shallow=False), (a, f)
    v4, d4 = u[:R * F].reshape(R, F, V, 3), r[:R * F].reshape(R, F, V)
    check_files(tmp_path / 'new', hostct.calculate_Ct_dipolar_cross(v4, pairs, dist=d4, ctx=ctx), pairs, names, np.float32(1.0), float(F))
    both = np.stack((pairs, pairs[:, ::-1]), axis=1).reshape(-1, 2)
    check_files(tmp_path / 'asym', hostct.calculate_Ct_dipolar_cross(v4, both, dist=d4, symmetric=False, ctx=ctx), both, names, np.float32(1.0),
                float(F))
    p = run('-s', 'none.pdb', '-f', fn, '--tau', F, '-o', str(tmp_path / 'o'), '--dipolarCrossCt')
    assert p.returncode != 0 and b'--pairs' in p.stdout
