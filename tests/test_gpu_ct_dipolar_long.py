"""
GPU tests (marker gpu) of the blocked forms of the two distance-weighted correlation functions (csrc/sr_ct_dipolar_long.hip: k_dipl_wsums,
k_dipl_f64 and the shared kernels of sr_ct_long.h / sr_ct_long.hip / sr_ct_cross_long.hip in their traceless, four-plane form) through
the _dev entry points, hip.ResidentVectors.ct_dipolar_long / ct_dipolar_cross_long, the dispatch of spinrelax_amd.ct and the --dipolarCt
flag of scripts/calculate-Ct-from-traj.py.

Inputs: make_pairs of tests/test_gpu_ct_dipolar.py; every case asserts that the reference C (and P0) is >= 0.4 at every lag, so the
relative bar means something.  The oracle is the definition by float64 numpy.fft correlations (tests/test_ct_dipolar_long_host.py,
held there to 1e-12 against the lag-by-lag oracles of the direct kernels' tests).
Bars, quoted from tests/test_gpu_ct_dipolar.py and tests/test_gpu_ct_dipolar_cross.py:
  * mode 0: relerr(C) < 1e-6, dct_close on dC, 1e-6 relative on reff6, reff3, S2rad and P0 (dct_close with 2 F on dP0);
  * mode 1 (float64 throughout) against the definition on the planes the pack wrote: 1e-12 absolute on C, dC and P0.
Measured on MI355X (mode 0, relerr of C): 1.8e-8 .. 2.0e-8 for the autocorrelation form at F = 10017 .. 20000, 1.9e-8 at F = 262144,
1.6e-8 .. 2.3e-8 for the pair form at F = 4097 .. 12289; mode 1 within 1e-14; docs/EXPERIMENTS.md has the table.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr
from test_ct_dipolar_long_host import fft_core, fft_cross_core, oracle_dcross_fft, oracle_dipolar_fft
from test_gpu_ct_cross import dct_close
from test_gpu_ct_dipolar import check_dipolar_files, dev_pack, make_pairs
from spinrelax_amd import ct as hostct
from spinrelax_amd.hip import SpinRelaxHipError

pytestmark = pytest.mark.gpu

RTOL = 1e-6
FLOOR = 0.4
PAIRS = np.array([(0, 0), (1, 2), (2, 1), (3, 1), (1, 2)], dtype=np.int32)
# (10017, 3): the first length the direct kernel refuses, odd F; (12288, 2): three full blocks, lag L at offset 1, m = 2048; (12289, 3): one
# sample in the last block; (16385, 2): nb = 5, nd = 3; (20000, 3): the general long case
AUTO = [(10017, 3), (12288, 2), (12289, 3), (16385, 2), (20000, 3)]
# (4897, 3): the first length the direct pair kernel refuses; (8192, 2): two full blocks, nd = 2; (8193, 3): one sample in the third
# block; (12289, 2): nb = 4, nd = 2
PAIR = [(4897, 3), (8192, 2), (8193, 3), (12289, 2)]


@pytest.fixture(scope='module')
def ctx():
    from spinrelax_amd.hip import Context
    c = Context(0)
    yield c
    c.close()


_cache = {}


def vectors(N, seed, nV):
    """make_pairs, computed once per (N, seed, nV) and never written to"""
    if (N, seed, nV) not in _cache:
        _cache[(N, seed, nV)] = make_pairs(N, seed=seed, nV=nV)
    return _cache[(N, seed, nV)]


def auto_case(F, R):
    if ('a', F, R) not in _cache:
        u, r, raw = vectors(R * F, 7000 + F % 1000 + R, 3)
        _cache[('a', F, R)] = (u, r, raw, oracle_dipolar_fft(raw, None, R, F))
    return _cache[('a', F, R)]


def pair_case(F, R):
    if ('p', F, R) not in _cache:
        u, r, raw = vectors(R * F, 8000 + F % 1000 + R, 4)
        _cache[('p', F, R)] = (u, r, raw, {s: oracle_dcross_fft(raw, None, PAIRS, s, R, F) for s in (0, 1)}, oracle_dipolar_fft(raw, None, R, F))
    return _cache[('p', F, R)]


def check_auto(label, got, ref, R, F):
    """the mode-0 bars on (C, dC, reff6, reff3, S2rad)"""
    assert ref[0].min() >= FLOOR, ref[0].min()
    L = F // 2
    print('%s F=%d R=%d: min C %.3f relerr C %.2e |d dC| %.2e reff6 %.2e reff3 %.2e S2rad %.2e' % (
        label, F, R, ref[0].min(), relerr(got[0], ref[0]), np.max(np.abs(got[1] - ref[1])), relerr(got[2], ref[2]), relerr(got[3], ref[3]),
        relerr(got[4], ref[4])))
    assert got[0].shape == got[1].shape == ref[0].shape == (L, ref[0].shape[1])
    assert relerr(got[0], ref[0]) < RTOL
    assert dct_close(got[1], ref[1], R, F)
    for g, w in zip(got[2:], ref[2:]):
        assert relerr(g, w) < RTOL


def check_pair(label, got, ref, R, F):
    """the mode-0 bars on (P0, dP0, C, dC, reff6)"""
    assert min(ref[0].min(), ref[2].min()) >= FLOOR, (ref[0].min(), ref[2].min())
    print('%s F=%d R=%d: min C %.3f relerr C %.2e P0 %.2e |d dC| %.2e |d dP0| %.2e reff6 %.2e' % (
        label, F, R, ref[2].min(), relerr(got[2], ref[2]), relerr(got[0], ref[0]), np.max(np.abs(got[3] - ref[3])),
        np.max(np.abs(got[1] - ref[1])), relerr(got[4], ref[4])))
    assert got[2].shape == got[3].shape == ref[2].shape
    assert relerr(got[2], ref[2]) < RTOL and relerr(got[0], ref[0]) < RTOL
    assert dct_close(got[3], ref[3], R, F) and dct_close(got[1], ref[1], R, 2 * F)
    assert relerr(got[4], ref[4]) < RTOL


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize('F,R', AUTO)
def test_autocorrelation_form_through_the_default_dispatch(ctx, F, R):
    u, r, raw, ref = auto_case(F, R)
    got = hostct.calculate_Ct_dipolar(raw.reshape(R, F, 3, 3), ctx=ctx, mode=0)
    check_auto('auto', got, ref, R, F)
    if F == 12289:
        # the work area in tiles of one series (1 MiB holds less than one: the tile is one series) against all series at once, and a
        # second run: the same bytes
        ctx.set_option('ct_long_ws_mb', 1)
        try:
            tiled = hostct.calculate_Ct_dipolar(raw.reshape(R, F, 3, 3), ctx=ctx, mode=0)
        finally:
            ctx.set_option('ct_long_ws_mb', 256)
        assert same_bytes(got, tiled)
        assert same_bytes(got, hostct.calculate_Ct_dipolar(raw.reshape(R, F, 3, 3), ctx=ctx, mode=0))
    if F == 10017:
        # the other input form: unit vectors and the distances beside them
        alt = hostct.calculate_Ct_dipolar(u.reshape(R, F, 3, 3), dist=r.reshape(R, F, 3), ctx=ctx, mode=0)
        check_auto('auto, dist given', alt, oracle_dipolar_fft(u, r, R, F), R, F)


def test_autocorrelation_form_on_irregular_chunks_with_an_odd_start(ctx):
    """chunk starts 0, F + 4 (odd) and 2 F + 11: the unaligned load path of k_ctl_spectra; r_ref runs over all frames held"""
    F, R = 10017, 3
    u, r, raw = vectors(3 * F + 16, 7100, 3)
    starts = np.array([0, F + 4, 2 * F + 11], dtype=np.int64)
    assert starts[1] % 2 == 1
    with ctx.vectors(3, raw.shape[0]) as rv:
        rv.append(raw)
        got = hostct.calculate_Ct_dipolar_resident(rv, R, F, chunk_start=starts)
        check_auto('auto, ragged', got, oracle_dipolar_fft(raw, None, R, F, starts), R, F)
        bad = starts.copy()
        bad[2] = raw.shape[0] - F + 1
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_dipolar_long(R, F, chunk_start=bad)
        assert '(-3)' in str(exc.value)


@pytest.mark.parametrize('sym', [0, 1])
@pytest.mark.parametrize('F,R', PAIR)
def test_pair_form_through_the_default_dispatch(ctx, F, R, sym):
    u, r, raw, refs, refa = pair_case(F, R)
    ref = refs[sym]
    got = hostct.calculate_Ct_dipolar_cross(raw.reshape(R, F, 4, 3), PAIRS, symmetric=bool(sym), ctx=ctx, mode=0)
    check_pair('pair sym=%d' % sym, got, ref, R, F)
    P0, dP0, C, dC, reff6 = got
    # the repeated pair: the same bytes
    assert C[:, 1].tobytes() == C[:, 4].tobytes() and dC[:, 1].tobytes() == dC[:, 4].tobytes()
    assert P0[1] == P0[4] and dP0[1].tobytes() == dP0[4].tobytes() and reff6[1].tobytes() == reff6[4].tobytes()
    if sym:
        assert C[:, 1].tobytes() == C[:, 2].tobytes()                      # (1, 2) and (2, 1) are one symmetric function
    else:
        assert np.max(np.abs(ref[2][:, 1] - ref[2][:, 2])) > 1e-4 and C[:, 1].tobytes() != C[:, 2].tobytes()
    # pair (0, 0) is the autocorrelation form's function, with P0 = 1
    auto = hostct.calculate_Ct_dipolar(raw.reshape(R, F, 4, 3), ctx=ctx, mode=0)
    if F > ctx.ct_dipolar_max_frames():
        check_auto('auto beside the pairs', auto, refa, R, F)
    print('pair (0, 0) against the autocorrelation form %.2e, P0 - 1 = %.2e' % (relerr(C[:, 0], auto[0][:, 0]), P0[0] - 1.0))
    assert relerr(C[:, 0], auto[0][:, 0]) < RTOL and abs(P0[0] - 1.0) < RTOL
    if F == 8193 and sym:
        ctx.set_option('ct_long_ws_mb', 1)
        try:
            tiled = hostct.calculate_Ct_dipolar_cross(raw.reshape(R, F, 4, 3), PAIRS, symmetric=True, ctx=ctx, mode=0)
        finally:
            ctx.set_option('ct_long_ws_mb', 256)
        assert same_bytes(got, tiled)


def test_float64_mode_of_the_autocorrelation_form(ctx):
    """mode 1 against the definition on the planes the pack wrote, through sr_ct_dipolar_long_f32_dev"""
    import torch
    F, R = 10017, 3
    u, r, raw, _ = auto_case(F, R)
    p, rref, planes, Npad = dev_pack(ctx, raw, None)
    L = F // 2
    Ct = torch.empty((L, 3), device='cuda', dtype=torch.float64)
    dCt = torch.empty((L, 3), device='cuda', dtype=torch.float64)
    wm = torch.empty((3, 2), device='cuda', dtype=torch.float64)
    a4 = p[:, :3, :R * F].transpose(2, 0, 1).reshape(R, F, 3, 3)
    w4 = p[:, 3, :R * F].T.reshape(R, F, 3)
    Cr, dCr, w1, w2 = fft_core(a4, w4)
    assert Cr.min() >= FLOOR
    for mode, bar in ((1, 1e-12), (0, None)):
        ctx.ct_dipolar_long_dev(planes.data_ptr(), Npad, 3, R, F, Ct.data_ptr(), dCt.data_ptr(), wm.data_ptr(), mode=mode)
        ctx.sync()
        C, dC, w = Ct.cpu().numpy(), dCt.cpu().numpy(), wm.cpu().numpy()
        print('mode %d on the planes: |dC| %.2e |d dC| %.2e relerr C %.2e <w> %.2e <w^2> %.2e' % (
            mode, np.max(np.abs(C - Cr)), np.max(np.abs(dC - dCr)), relerr(C, Cr), relerr(w[:, 0], w1), relerr(w[:, 1], w2)))
        assert relerr(w[:, 0], w1) <= 1e-12 and relerr(w[:, 1], w2) <= 1e-12
        if mode == 1:
            assert np.max(np.abs(C - Cr)) <= bar and np.max(np.abs(dC - dCr)) <= bar
        else:
            assert relerr(C, Cr) < RTOL and dct_close(dC, dCr, R, F)


def test_float64_mode_of_the_pair_form(ctx):
    """mode 1 against the definition on the planes the pack wrote, through sr_ct_dipolar_cross_long_f32_dev, sym = 0 and 1"""
    import torch
    F, R = 4897, 3
    u, r, raw, _, _ = pair_case(F, R)
    p, rref, planes, Npad = dev_pack(ctx, raw, None)
    L, nP = F // 2, len(PAIRS)
    P0 = torch.empty((2, nP), device='cuda', dtype=torch.float64)
    Ct = torch.empty((L, nP), device='cuda', dtype=torch.float64)
    dCt = torch.empty((L, nP), device='cuda', dtype=torch.float64)
    ws = torch.empty((nP, R, 2), device='cuda', dtype=torch.float64)
    a4 = p[:, :3, :R * F].transpose(2, 0, 1).reshape(R, F, 4, 3)
    w4 = p[:, 3, :R * F].T.reshape(R, F, 4).astype(np.float64)
    for sym in (0, 1):
        ref = fft_cross_core(a4, w4, PAIRS, sym)
        assert min(ref[0].min(), ref[2].min()) >= FLOOR
        for mode in (1, 0):
            ctx.ct_dipolar_cross_long_dev(planes.data_ptr(), Npad, 4, R, F, PAIRS, P0[0].data_ptr(), Ct.data_ptr(), dCt.data_ptr(), ws.data_ptr(),
                                          sym=sym, mode=mode, dP0_ptr=P0[1].data_ptr())
            ctx.sync()
            P, C, dC, w = P0.cpu().numpy(), Ct.cpu().numpy(), dCt.cpu().numpy(), ws.cpu().numpy()
            print('sym %d mode %d on the planes: |dC| %.2e |d dC| %.2e |dP0| %.2e |d dP0| %.2e' % (
                sym, mode, np.max(np.abs(C - ref[2])), np.max(np.abs(dC - ref[3])), np.max(np.abs(P[0] - ref[0])), np.max(np.abs(P[1] - ref[1]))))
            w2 = (w4 ** 2).sum(axis=1)                                         # (R, V)
            assert relerr(w[:, :, 0], w2[:, PAIRS[:, 0]].T) <= 1e-12 and relerr(w[:, :, 1], w2[:, PAIRS[:, 1]].T) <= 1e-12
            if mode == 1:
                assert np.max(np.abs(C - ref[2])) <= 1e-12 and np.max(np.abs(dC - ref[3])) <= 1e-12
                assert np.max(np.abs(P[0] - ref[0])) <= 1e-12 and np.max(np.abs(P[1] - ref[1])) <= 1e-12
            else:
                assert relerr(C, ref[2]) < RTOL and relerr(P[0], ref[0]) < RTOL
                assert dct_close(dC, ref[3], R, F) and dct_close(P[1], ref[1], R, 2 * F)


@pytest.mark.parametrize('F', [5462, 10016])
def test_both_kernels_of_the_autocorrelation_form_at_one_length(ctx, F):
    R = 2
    u, r, raw = vectors(R * F, 7200 + F % 1000, 3)
    ref = oracle_dipolar_fft(raw, None, R, F)
    v4 = raw.reshape(R, F, 3, 3)
    assert ctx.ct_dipolar_long_min_frames == 10017
    direct = hostct.calculate_Ct_dipolar(v4, ctx=ctx)
    with pytest.raises(SpinRelaxHipError) as exc:
        ctx.set_option('ct_dipolar_long_min_frames', 5461)                 # below the floor
    assert '(-3)' in str(exc.value) and ctx.ct_dipolar_long_min_frames == 10017
    ctx.set_option('ct_dipolar_long_min_frames', 5462)
    try:
        blocked = hostct.calculate_Ct_dipolar(v4, ctx=ctx)
    finally:
        ctx.set_option('ct_dipolar_long_min_frames', 10017)
    check_auto('direct ', direct, ref, R, F)
    check_auto('blocked', blocked, ref, R, F)
    print('blocked against direct: relerr C %.2e' % relerr(blocked[0], direct[0]))
    assert relerr(blocked[0], direct[0]) < RTOL and dct_close(blocked[1], direct[1], R, F)
    assert blocked[0].tobytes() != direct[0].tobytes()                     # two kernels: the dispatch took the blocked form
    assert same_bytes(direct, hostct.calculate_Ct_dipolar(v4, ctx=ctx))    # and the restored option gives the direct one again


@pytest.mark.parametrize('F', [4097, 4896])
def test_both_kernels_of_the_pair_form_at_one_length(ctx, F):
    R = 2
    u, r, raw = vectors(R * F, 8200 + F % 1000, 4)
    v4 = raw.reshape(R, F, 4, 3)
    assert ctx.ct_dipolar_cross_long_min_frames == 4897
    with pytest.raises(SpinRelaxHipError) as exc:
        ctx.set_option('ct_dipolar_cross_long_min_frames', 4096)           # below the floor
    assert '(-3)' in str(exc.value) and ctx.ct_dipolar_cross_long_min_frames == 4897
    for sym in (0, 1):
        ref = oracle_dcross_fft(raw, None, PAIRS, sym, R, F)
        direct = hostct.calculate_Ct_dipolar_cross(v4, PAIRS, symmetric=bool(sym), ctx=ctx)
        ctx.set_option('ct_dipolar_cross_long_min_frames', 4097)
        try:
            blocked = hostct.calculate_Ct_dipolar_cross(v4, PAIRS, symmetric=bool(sym), ctx=ctx)
        finally:
            ctx.set_option('ct_dipolar_cross_long_min_frames', 4897)
        check_pair('direct  sym=%d' % sym, direct, ref, R, F)
        check_pair('blocked sym=%d' % sym, blocked, ref, R, F)
        print('blocked against direct: relerr C %.2e P0 %.2e' % (relerr(blocked[2], direct[2]), relerr(blocked[0], direct[0])))
        assert relerr(blocked[2], direct[2]) < RTOL and relerr(blocked[0], direct[0]) < RTOL
        assert dct_close(blocked[3], direct[3], R, F) and dct_close(blocked[1], direct[1], R, 2 * F)
        assert blocked[2].tobytes() != direct[2].tobytes()
        assert same_bytes(direct, hostct.calculate_Ct_dipolar_cross(v4, PAIRS, symmetric=bool(sym), ctx=ctx))


def test_longest_chunk(ctx):
    """F = 262144, R = 2, one vector: nb = 64, nd = 33"""
    F, R = 262144, 2
    assert ctx.ct_dipolar_long_max_frames() == F and ctx.ct_dipolar_cross_long_max_frames() == F
    u, r, raw = vectors(R * F, 7300, 1)
    ref = oracle_dipolar_fft(raw, None, R, F)
    got = hostct.calculate_Ct_dipolar(raw.reshape(R, F, 1, 3), ctx=ctx)
    check_auto('longest', got, ref, R, F)


def test_refusals(ctx):
    """-4 beyond 262144 frames, -3 where the direct forms return -3 and below the floors; the direct entry points keep refusing the
    lengths the blocked ones take"""
    F = 262145
    pairs = np.array([(0, 1)], dtype=np.int32)
    with ctx.vectors(2, F) as rv:
        rv.append(np.tile(np.array([[[0.3, 0.0, 0.1], [0.0, 0.2, 0.2]]], dtype=np.float32), (F, 1, 1)))
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_dipolar_long(1, F)
        assert '(-4)' in str(exc.value) and '262144' in str(exc.value)
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_dipolar_cross_long(1, F, pairs)
        assert '(-4)' in str(exc.value) and '262144' in str(exc.value)
        with pytest.raises(ValueError):
            hostct.calculate_Ct_dipolar_resident(rv, 1, F)
        with pytest.raises(ValueError):
            hostct.calculate_Ct_dipolar_cross_resident(rv, pairs, 1, F)
    u, r, raw = vectors(3 * 10017 + 16, 7100, 3)
    with ctx.vectors(3, raw.shape[0]) as rv:
        rv.append(raw)
        # the direct entry points keep their limits, the blocked ones take these lengths
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_dipolar(1, 10017)
        assert '(-4)' in str(exc.value) and '10016' in str(exc.value)
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_dipolar_cross(1, 4897, pairs)
        assert '(-4)' in str(exc.value) and '4896' in str(exc.value)
        assert rv.ct_dipolar_long(1, 10017)[0].shape == (5008, 3)
        assert rv.ct_dipolar_cross_long(1, 4897, pairs)[2].shape == (2448, 1)
        for call in (lambda: rv.ct_dipolar_long(1, 5461),                                  # below the floors
                     lambda: rv.ct_dipolar_cross_long(1, 4096, pairs),
                     lambda: rv.ct_dipolar_long(1, 10017, mode=2),                         # mode, sym
                     lambda: rv.ct_dipolar_cross_long(1, 4897, pairs, mode=2),
                     lambda: rv.ct_dipolar_cross_long(1, 4897, pairs, sym=2),
                     lambda: rv.ct_dipolar_long(4, 10017),                                 # more chunks than frames held
                     lambda: rv.ct_dipolar_cross_long(7, 4897, pairs),
                     lambda: rv.ct_dipolar_long(0, 10017),
                     lambda: rv.ct_dipolar_cross_long(1, 4897, [(0, 3)]),                  # a pair outside the vectors
                     lambda: rv.ct_dipolar_long(1, 10017, dist=-np.ones((raw.shape[0], 3), dtype=np.float32))):
            with pytest.raises(SpinRelaxHipError) as exc:
                call()
            assert '(-3)' in str(exc.value), str(exc.value)
    bad = raw[:10017].copy()
    bad[40, 2] = 0.0
    with ctx.vectors(3, 10017) as rv:
        rv.append(bad)
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_dipolar_long(1, 10017)
        assert '(-3)' in str(exc.value) and 'vector 2' in str(exc.value)


def test_cli_dipolarCt_with_a_long_memory_time(tmp_path, ctx):
    """--dipolarCt with a --tau of 10017 frames writes its two files, which agree with the API in the digits they keep"""
    F, R, V = 10017, 2, 3
    u, r, raw = vectors(R * F + 5, 7400, V)
    names = np.arange(11, 11 + V)
    fn = str(tmp_path / 'pairs.npz')
    np.savez(fn, vecs=u, dist=r, names=names, dt=1.0)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py'), '-s', 'none.pdb', '-f', fn, '--tau', str(F),
                        '-o', str(tmp_path / 'o'), '--dipolarCt'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    assert sorted(os.listdir(str(tmp_path))) == ['o_dipolarCtint.dat', 'o_dipolarDist.dat', 'pairs.npz']
    want = hostct.calculate_Ct_dipolar(u[:R * F].reshape(R, F, V, 3), dist=r[:R * F].reshape(R, F, V), ctx=ctx)
    check_auto('cli', want, oracle_dipolar_fft(u[:R * F], r[:R * F], R, F), R, F)
    check_dipolar_files(tmp_path, want, names, np.float32(1.0), float(F))
