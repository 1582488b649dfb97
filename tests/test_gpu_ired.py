"""
GPU tests of the iRED matrix kernels (csrc/sr_ired.hip) and of everything above them: hip.ResidentVectors.ired, spinrelax_amd.ired
and the --iRED flags of scripts/calculate-Ct-from-traj.py.

Oracle (in this file): the literal definition in float64 numpy on the same float32 vectors,
    M[i][j] = (1/F) sum_t ( 1.5 (u_i(t).u_j(t))^2 - 0.5 )   with   einsum('tia,tja->tij'),   then numpy.linalg.eigh.

Bars.  M: 1e-11 absolute for every split setting (worst-case chain bound K 2^-53 sum|terms| / F <= 6 * 1536 * 1.1e-16 * 1.5 =
1.5e-12 for the longest case here; expected ~1e-15).  S2 and dS2: 1e-8 absolute; every case first asserts that its oracle has
lambda_5 - lambda_6 >= 0.5, with which the perturbation of the global subspace, 2 |dM| / gap, stays below the bar.

Inputs: fixed body vectors, rotated by a random walk of the whole body (steps ~0.15 rad), every vector with an AR(1) wobble
(coefficient 0.9) of its own size sigma_i = 0.05 .. 0.5, renormalised, cast to float32.
"""
import filecmp
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, files_equal_numeric
from spinrelax_amd import general_scripts as gs
from spinrelax_amd import hip, ired
from spinrelax_amd._lib import SpinRelaxHipError

pytestmark = pytest.mark.gpu

BAR_M = 1e-11
BAR_S2 = 1e-8
MIN_GAP = 0.5


@functools.lru_cache(maxsize=None)
def make_vectors(N, F, wobble=True):
    rng = np.random.default_rng(1000 * N + F)
    b = rng.standard_normal((N, 3))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    R = np.empty((F, 3, 3))
    cur = np.eye(3)
    for t in range(F):
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        ang = 0.15 * rng.standard_normal()
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        cur = cur @ (np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K))
        R[t] = cur
    sig = (np.linspace(0.05, 0.5, N) if wobble else np.zeros(N))[:, None]
    w = np.empty((F, N, 3))
    x = sig * rng.standard_normal((N, 3))
    for t in range(F):
        x = 0.9 * x + np.sqrt(1 - 0.81) * sig * rng.standard_normal((N, 3))
        w[t] = x
    v = np.einsum('tab,tnb->tna', R, b[None] + w)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    v = v.astype(np.float32)
    v.setflags(write=False)
    return v


def oracle_M(v, start, length):
    u = np.asarray(v[start:start + length], dtype=np.float64)
    d = np.einsum('tia,tja->tij', u, u)
    return (1.5 * d * d - 0.5).sum(axis=0) / length


def oracle_S2(M, G=5):
    """S2 (N), lambda descending (N); asserts the gap the S2 bar rests on"""
    lam, vec = np.linalg.eigh(M)
    lam, vec = lam[::-1], vec[:, ::-1]
    assert lam[G - 1] - lam[G] >= MIN_GAP, 'oracle gap %.3g' % (lam[G - 1] - lam[G])
    return 1.0 - (lam[G:] * vec[:, G:] ** 2).sum(axis=1), lam


def oracle_reduce(S2_w):
    W = S2_w.shape[0]
    return S2_w.mean(axis=0), (S2_w.std(axis=0) / (np.sqrt(W) - 1.0) if W > 1 else np.zeros(S2_w.shape[1]))


@pytest.fixture(scope='module')
def ctx():
    c = hip.Context()
    yield c
    c.close()


def gpu_M(ctx, v, starts, lens):
    with ctx.vectors(v.shape[1], v.shape[0]) as rv:
        rv.append(v)
        return rv.ired(starts, lens)


@pytest.mark.parametrize('N,F', [(6, 3), (24, 1536), (37, 1000), (64, 512), (70, 777)])
def test_shapes_one_window(ctx, N, F):
    """(6, 3): shorter than one MFMA k-step, minimal N; then a ragged single tile, an exact tile and two tiles with a ragged
    edge, whose off-diagonal tile block is not symmetric (a row / column swap of the accumulator map shows there)"""
    v = make_vectors(N, F)
    M = gpu_M(ctx, v, [0], [F])
    ref = oracle_M(v, 0, F)
    assert M.shape == (1, N, N)
    err = np.max(np.abs(M[0] - ref))
    print('N=%d F=%d max |dM| = %.3g' % (N, F, err))
    assert err < BAR_M
    if N >= 24:
        S2, lam = ired.ired_S2(M)
        S2_ref, lam_ref = oracle_S2(ref)
        assert np.max(np.abs(S2[0] - S2_ref)) < BAR_S2
        assert np.max(np.abs(lam[0] - lam_ref)) < BAR_S2


def test_windows_unaligned_and_unequal(ctx):
    v = make_vectors(70, 777)
    wins = [(1, 300), (301, 7), (308, 469)]
    M = gpu_M(ctx, v, [a for a, _ in wins], [n for _, n in wins])
    for w, (a, n) in enumerate(wins):
        ref = oracle_M(v, a, n)
        assert np.max(np.abs(M[w] - ref)) < BAR_M, wins[w]
        assert np.max(np.abs(ired.ired_S2(M[w])[0][0] - oracle_S2(ref)[0])) < BAR_S2, wins[w]


def test_windows_through_two_files(ctx):
    """two files, windows of 300 frames from ired_windows: the second file's windows start at its first frame, the tails of
    both are dropped"""
    v = make_vectors(70, 777)
    files = [v[:400], v[400:]]
    res = ired.calculate_iRED(files, dt=2.0, window=600.0, ctx=ctx)
    assert res['win_start'].tolist() == [0, 400] and res['win_len'].tolist() == [300, 300]
    refs = [oracle_M(v, 0, 300), oracle_M(v, 400, 300)]
    for w in range(2):
        assert np.max(np.abs(res['M'][w] - refs[w])) < BAR_M
    S2_w = np.stack([oracle_S2(r)[0] for r in refs])
    S2, dS2 = oracle_reduce(S2_w)
    assert np.max(np.abs(res['S2'] - S2)) < BAR_S2 and np.max(np.abs(res['dS2'] - dS2)) < BAR_S2


def test_forced_split_meets_the_bar_and_is_reproducible(ctx):
    v = make_vectors(37, 1000)
    ref = oracle_M(v, 0, 1000)
    try:
        for s in (1, 2, 3, 0):
            ctx.set_option('ired_ksplit', s)
            a = gpu_M(ctx, v, [0], [1000])
            b = gpu_M(ctx, v, [0], [1000])
            err = np.max(np.abs(a[0] - ref))
            print('ired_ksplit=%d max |dM| = %.3g' % (s, err))
            assert err < BAR_M, s
            assert a.tobytes() == b.tobytes(), s
    finally:
        ctx.set_option('ired_ksplit', 0)
    with pytest.raises(SpinRelaxHipError):
        ctx.set_option('ired_ksplit', -1)


def test_zero_vectors_contribute_minus_one_half(ctx):
    """vecnorm_NDarray turns 0/0 into (0, 0, 0): such a frame adds 1.5 * 0 - 0.5 to every pair it is in, the diagonal included"""
    v = make_vectors(37, 1000).copy()
    v[10:20, 3] = 0.0
    M = gpu_M(ctx, v, [0], [1000])
    ref = oracle_M(v, 0, 1000)
    assert abs(ref[3, 3] - (1.0 - 1.5 * 10 / 1000)) < 1e-6
    assert np.max(np.abs(M[0] - ref)) < BAR_M


@pytest.mark.parametrize('N,F', [(37, 1000), (70, 777)])
def test_symmetry_and_unit_diagonal(ctx, N, F):
    M = gpu_M(ctx, make_vectors(N, F), [0, 5], [F, F - 5])
    for w in range(2):
        assert np.array_equal(M[w], M[w].T)
        assert np.max(np.abs(np.diag(M[w]) - 1.0)) < 1e-6          # the float32 norm error of the inputs


def test_rigid_tumbling_gives_S2_one(ctx):
    v = make_vectors(24, 1536, wobble=False)
    res = ired.calculate_iRED([v], dt=1.0, ctx=ctx)
    assert res['win_len'].tolist() == [1536]
    assert np.max(np.abs(res['S2'] - 1.0)) < 1e-6
    assert np.max(np.abs(res['eig'][5:])) < 1e-6
    assert np.array_equal(res['dS2'], np.zeros(24))


def test_calculate_iRED_against_the_oracle(ctx):
    v = make_vectors(24, 1536)
    res = ired.calculate_iRED([v], dt=10.0, window=3840.0, ctx=ctx)
    assert res['win_start'].tolist() == [0, 384, 768, 1152] and res['win_len'].tolist() == [384] * 4
    per = [oracle_S2(oracle_M(v, a, 384)) for a in (0, 384, 768, 1152)]
    S2, dS2 = oracle_reduce(np.stack([p[0] for p in per]))
    lam = np.stack([p[1] for p in per]).mean(axis=0)
    assert np.max(np.abs(res['S2'] - S2)) < BAR_S2
    assert np.max(np.abs(res['dS2'] - dS2)) < BAR_S2
    assert np.max(np.abs(res['eig'] - lam)) < BAR_S2
    # the default window with a memory time: 5 tau
    res5 = ired.calculate_iRED([v], dt=10.0, tau=768.0, ctx=ctx)
    assert res5['win_start'].tolist() == [0, 384, 768, 1152]
    assert res5['M'].tobytes() == res['M'].tobytes()


def test_cli_iRED_outputs_and_nothing_else_changes(tmp_path):
    v = make_vectors(24, 1536)
    fn = str(tmp_path / 'vecs.npy')
    np.save(fn, v)
    script = os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')
    common = ['-s', 'none.pdb', '-f', fn, '--dt', '10', '--tau', '1280', '--Ct', '--S2', '--vecAvg', '--vecHist', '--binary']
    outs = []
    for name, extra in (('plain', []), ('ired', ['--iRED', '--iRED_window', '3840'])):
        d = tmp_path / name
        d.mkdir()
        p = subprocess.run([sys.executable, script] + common + ['-o', str(d / 'o')] + extra, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()[-3000:]
        outs.append(d)
    plain, withired = (sorted(os.listdir(str(d))) for d in outs)
    new = ['o_iRED_S2.dat', 'o_iRED_eig.dat', 'o_iRED_matrix.npz']
    assert len(plain) >= 5 and sorted(plain + new) == withired
    for f in plain:
        if f.endswith('.npz'):                  # a zip archive stamps its members with the time of writing: the arrays, bit for bit
            za, zb = (np.load(str(d / f), allow_pickle=True) for d in outs)
            assert sorted(za.files) == sorted(zb.files)
            for k in za.files:
                a, b = za[k], zb[k]
                assert a.dtype == b.dtype and a.shape == b.shape, (f, k)
                if a.dtype == object:
                    assert all(np.array_equal(x, y) for x, y in zip(a.ravel(), b.ravel())), (f, k)
                else:
                    assert a.tobytes() == b.tobytes(), (f, k)
        else:
            assert filecmp.cmp(str(outs[0] / f), str(outs[1] / f), shallow=False), f
    # the new files against the oracle
    z = np.load(str(outs[1] / 'o_iRED_matrix.npz'))
    assert z['win_start'].tolist() == [0, 384, 768, 1152] and z['win_len'].tolist() == [384] * 4
    assert z['resid'].tolist() == list(range(2, 26))
    refs = [oracle_M(v, a, 384) for a in (0, 384, 768, 1152)]
    assert np.max(np.abs(z['M'] - np.stack(refs))) < BAR_M
    per = [oracle_S2(r) for r in refs]
    S2, dS2 = oracle_reduce(np.stack([p[0] for p in per]))
    zeta = (1.02 / 1.04) ** 6
    gs.print_xylist(str(tmp_path / 'ref_S2.dat'), list(range(2, 26)), np.stack((S2, dS2)) * zeta, True)
    gs.print_xylist(str(tmp_path / 'ref_eig.dat'), np.arange(1, 25), np.stack([p[1] for p in per]).mean(axis=0)[None], True)
    # the text carries six digits: equal line by line, a last printed digit on a rounding boundary apart
    for mine, ref in (('o_iRED_S2.dat', 'ref_S2.dat'), ('o_iRED_eig.dat', 'ref_eig.dat')):
        ok, why = files_equal_numeric(str(outs[1] / mine), str(tmp_path / ref), rtol=2e-6)
        assert ok, (mine, why)
    got = np.loadtxt(str(outs[1] / 'o_iRED_S2.dat'), comments='&')
    assert got.shape == (24, 3) and np.max(np.abs(got[:, 1] - S2 * zeta)) < 1e-6


def test_refusals(ctx):
    v = make_vectors(37, 1000)
    with ctx.vectors(37, 1000) as rv:
        rv.append(v)
        with pytest.raises(SpinRelaxHipError):
            rv.ired([], [])                                         # W = 0
        with pytest.raises(SpinRelaxHipError):
            rv.ired([0, 900], [500, 101])                           # past the frames held
        with pytest.raises(SpinRelaxHipError):
            rv.ired([0], [0])                                       # an empty window
        with pytest.raises(SpinRelaxHipError):
            rv.ired([-1], [10])
        assert rv.ired([900], [100]).shape == (1, 37, 37)           # the last frame itself is fine
    with pytest.raises(ValueError):
        ired.calculate_iRED([v[:, :5]], dt=1.0, ctx=ctx)            # N = 5 does not exceed G = 5
    with pytest.raises(ValueError):
        ired.calculate_iRED([v], dt=1.0, window=2000.0, ctx=ctx)    # no file holds a window
