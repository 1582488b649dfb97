"""
GPU tests of the iRED mode correlation kernels (csrc/sr_ired_modes.hip: k_ired_project, k_ired_mode_ct) and of everything above
them: hip.ResidentVectors.ired_mode_ct, spinrelax_amd.ired (mode_ct=True) and the --iRED_Ct flag of scripts/calculate-Ct-from-traj.py.

Oracle (in this file): float64 numpy on the same float32 vectors, no FFT,
    A = einsum('mi,tic->tmc', coef, P),  P = (xx, yy, zz, xy, xz, yz),  w = (1, 1, 1, 2, 2, 2)
    C_m(k) = 1.5 / (F - k) * (A[:F-k] * A[k:] * w).sum() - 0.5 (sum_i e_mi)^2        every lag a direct dot product.
Coefficient matrices are random (default_rng, standard normal / sqrt(N)) unless a test says otherwise: nothing depends on an
eigen-solver's signs or on degenerate modes.

Bar.  |dC_m(k)| <= 1e-11 max(1, scale_m), scale_m = C_m(0) + 0.5 sigma_m^2 from the oracle.  Worst-case chain for the largest case
(N = 70): amplitudes N 2^-53 sum_i |e_mi| ~ 7e-14 relative, transforms ~13 stages x 2^-53, a factor <= 2 from 1 / (F - k) at
k <= F / 2: about 1e-12 scale in all; expected ~1e-14.  Every case prints its measured maximum.

Inputs: the generator of test_gpu_ired.py (fixed body vectors, a random walk of the whole body, an AR(1) wobble per vector,
renormalised, float32).
"""
import filecmp
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from spinrelax_amd import general_scripts as gs
from spinrelax_amd import hip, ired
from spinrelax_amd._lib import SpinRelaxHipError

pytestmark = pytest.mark.gpu

BAR = 1e-11
W6 = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])


@functools.lru_cache(maxsize=None)
def make_vectors(N, F, seed=None):
    rng = np.random.default_rng(1000 * N + F if seed is None else seed)
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
    sig = np.linspace(0.05, 0.5, N)[:, None]
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


def random_coef(W, K, N, seed):
    return np.random.default_rng(seed).standard_normal((W, K, N)) / np.sqrt(N)


def oracle_Cm(v, start, F, coef, n_lags):
    """coef (K, N) -> C (K, n_lags), scale (K)"""
    u = np.asarray(v[start:start + F], dtype=np.float64)
    x, y, z = u[..., 0], u[..., 1], u[..., 2]
    P = np.stack((x * x, y * y, z * z, x * y, x * z, y * z), axis=-1)
    A = np.einsum('mi,tic->tmc', coef, P)
    Aw = A * W6
    sig = coef.sum(axis=1)
    C = np.empty((coef.shape[0], n_lags))
    for k in range(n_lags):
        C[:, k] = 1.5 / (F - k) * (A[:F - k] * Aw[k:]).sum(axis=(0, 2)) - 0.5 * sig * sig
    return C, C[:, 0] + 0.5 * sig * sig


def oracle_M(v, start, length):
    u = np.asarray(v[start:start + length], dtype=np.float64)
    d = np.einsum('tia,tja->tij', u, u)
    return (1.5 * d * d - 0.5).sum(axis=0) / length


def oracle_tau(C, dt):
    tau = np.zeros(C.shape[0])
    for m, c in enumerate(C):
        if c[0] <= 0:
            continue
        n = len(c)
        for k in range(len(c)):
            if c[k] <= 0:
                n = k
                break
        tau[m] = dt * sum(0.5 * (c[k] + c[k + 1]) for k in range(n - 1)) / c[0]
    return tau


def worst(got, ref, scale):
    """max over (m, k) of |got - ref| / max(1, scale_m)"""
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, scale)[:, None]))


@pytest.fixture(scope='module')
def ctx():
    c = hip.Context()
    yield c
    c.close()


def gpu_Cm(ctx, v, starts, lens, coef, n_lags):
    with ctx.vectors(v.shape[1], v.shape[0]) as rv:
        rv.append(v)
        return rv.ired_mode_ct(starts, lens, coef, n_lags)


@pytest.mark.parametrize('N,K,F,n_lags', [(6, 6, 3, 2), (37, 5, 700, 351), (24, 24, 1536, 769), (64, 64, 512, 257), (70, 70, 777, 389),
                                          (24, 8, 3000, 1501), (24, 8, 5000, 2501), (8, 4, 5461, 2731)])
def test_shapes_one_window(ctx, N, K, F, n_lags):
    """(6, 6, 3, 2): shorter than one k-step; (37, 5, 700): ragged N, K < 16, padded to 2048 points; (24, 24, 1536): M = 4096;
    (64, 64, 512): exact tiles; (70, 70, 777): two mode tiles and ragged vector stages -- the coefficient matrix is not symmetric,
    a swapped accumulator map shows; then M = 6144, M = 8192 and need = 8191, the boundary.
    Measured max |dC| / max(1, scale) on the MI355X: see docs/EXPERIMENTS.md section 19."""
    v = make_vectors(N, F)
    coef = random_coef(1, K, N, seed=N * 7919 + K)
    C = gpu_Cm(ctx, v, [0], [F], coef, n_lags)
    assert C.shape == (1, K, n_lags)
    ref, scale = oracle_Cm(v, 0, F, coef[0], n_lags)
    err = worst(C[0], ref, scale)
    print('N=%d K=%d F=%d n_lags=%d max |dC|/max(1,scale) = %.3g' % (N, K, F, n_lags, err))
    assert err <= BAR


def test_windows_unaligned_with_gaps(ctx):
    """three windows of 500 frames at 0, 513 and 1101 of 1700, a coefficient matrix per window: each equals its one-window call
    bit for bit, and the oracle"""
    v = make_vectors(37, 1700)
    starts, lens = [0, 513, 1101], [500, 500, 500]
    coef = random_coef(3, 37, 37, seed=11)
    with ctx.vectors(37, 1700) as rv:
        rv.append(v)
        C = rv.ired_mode_ct(starts, lens, coef, 251)
        for w in range(3):
            one = rv.ired_mode_ct(starts[w:w + 1], lens[w:w + 1], coef[w:w + 1], 251)
            assert one[0].tobytes() == C[w].tobytes(), w
    for w in range(3):
        ref, scale = oracle_Cm(v, starts[w], 500, coef[w], 251)
        err = worst(C[w], ref, scale)
        print('window %d max |dC|/max(1,scale) = %.3g' % (w, err))
        assert err <= BAR


def test_work_area_batching_changes_nothing(ctx):
    """6 windows of 700 frames, K = 37: 48 * 37 * 700 B = 1.2 MB of amplitudes per window, so ired_ws_mb = 1 gives one window per
    batch, the default all six in one"""
    v = make_vectors(37, 4200)
    starts, lens = np.arange(6) * 700, np.full(6, 700)
    coef = random_coef(6, 37, 37, seed=12)
    with ctx.vectors(37, 4200) as rv:
        rv.append(v)
        try:
            ctx.set_option('ired_ws_mb', 1)
            small = rv.ired_mode_ct(starts, lens, coef, 351)
        finally:
            ctx.set_option('ired_ws_mb', 1024)
        big = rv.ired_mode_ct(starts, lens, coef, 351)
        again = rv.ired_mode_ct(starts, lens, coef, 351)
    assert small.tobytes() == big.tobytes()
    assert again.tobytes() == big.tobytes()
    ref, scale = oracle_Cm(v, 3500, 700, coef[5], 351)
    assert worst(big[5], ref, scale) <= BAR
    with pytest.raises(SpinRelaxHipError):
        ctx.set_option('ired_ws_mb', 0)


def test_eigenmode_identities(ctx):
    """rows = eigenvectors of the window's own M: C_m(0) = lambda_m and sum_m |m>_i^2 C_m(0) = M_ii"""
    v = make_vectors(24, 1536)
    with ctx.vectors(24, 1536) as rv:
        rv.append(v)
        M = rv.ired([0], [1536])
        lam, vec = np.linalg.eigh(M[0])
        C = rv.ired_mode_ct([0], [1536], vec.T[None], 1)
    e1 = np.max(np.abs(C[0, :, 0] - lam))
    e2 = np.max(np.abs(ired.ired_vector_ct(vec, C[0])[:, 0] - np.diag(M[0])))
    print('max |C_m(0) - lambda_m| = %.3g, max |sum_m vec^2 C_m(0) - M_ii| = %.3g' % (e1, e2))
    assert e1 <= 1e-10 and e2 <= 1e-10


def test_refusals(ctx):
    v = make_vectors(8, 5462)
    coef = random_coef(1, 4, 8, seed=13)
    with ctx.vectors(8, 5462) as rv:
        rv.append(v)
        for args, code, word in ((([0], [5462], coef, 2732), -4, '8192'),              # 5462 + 2732 - 1 = 8193
                                 (([0], [100], coef, 101), -3, 'n_lags'),
                                 (([0], [100], coef[:, :0], 10), -3, 'K='),
                                 (([5400], [63], coef, 10), -3, 'window 0'),               # one frame past the 5462 held
                                 (([0], [100], coef, 0), -3, 'n_lags')):
            with pytest.raises(SpinRelaxHipError) as exc:
                rv.ired_mode_ct(*args)
            assert '(%d)' % code in str(exc.value) and word in str(exc.value), (str(exc.value), code, word)
        assert rv.ired_mode_ct([5400], [62], coef, 10).shape == (1, 4, 10)              # the last frame itself is fine
        with pytest.raises(ValueError):
            rv.ired_mode_ct([0], [100], coef[:, :, :7], 10)                             # coefficient rows of the wrong length


SEED_TWO_FILES = 2400                  # chosen on the CPU: the oracle eigenvalues of all four windows are >= 1e-6 apart


def test_calculate_iRED_mode_ct_against_the_oracle(ctx):
    """two files of 1100 and 1300 frames, windows of 500: Ct_vec, dCt_vec and tau against the oracle fed numpy.linalg.eigh of the
    GPU's own M (the modes enter squared: signs cancel).  Bars: Ct_vec 1e-9; dCt_vec 2e-9 (a standard deviation moves by at most
    twice the largest change of a sample; sqrt(W) - 1 = 1 here); tau_m 2 dt n_lags 1e-9 / C_m(0) (every term C_m(k) / C_m(0) of the sum moves by at
    most 1e-9 (1 + |C_m(k)| / C_m(0)) / C_m(0) <= 2e-9 / C_m(0))."""
    v = make_vectors(24, 2400, seed=SEED_TWO_FILES)
    files = [v[:1100], v[1100:]]
    dt = 2.0
    res = ired.calculate_iRED(files, dt=dt, window=1000.0, ctx=ctx, mode_ct=True)
    assert res['win_start'].tolist() == [0, 500, 1100, 1600] and res['win_len'].tolist() == [500] * 4
    n_lags = 251
    assert res['Cm_w'].shape == (4, 24, n_lags) and res['Ct_vec'].shape == (n_lags, 24) and res['tau'].shape == (24,)
    Cm_w, Ct_w = [], []
    for w, a in enumerate((0, 500, 1100, 1600)):
        lam, vec = np.linalg.eigh(res['M'][w])
        lam, vec = lam[::-1], vec[:, ::-1]
        assert np.min(-np.diff(lam)) >= 1e-6, 'window %d: oracle eigenvalues %.3g apart' % (w, np.min(-np.diff(lam)))
        C, _ = oracle_Cm(v, a, 500, vec.T, n_lags)
        Cm_w.append(C)
        Ct_w.append(np.einsum('im,mk->ik', vec * vec, C))
    Cm, Ct_w = np.mean(Cm_w, axis=0), np.stack(Ct_w)
    Ct, dCt = Ct_w.mean(axis=0).T, (Ct_w.std(axis=0) / (np.sqrt(4) - 1.0)).T
    tau = oracle_tau(Cm, dt)
    e_ct, e_dct = np.max(np.abs(res['Ct_vec'] - Ct)), np.max(np.abs(res['dCt_vec'] - dCt))
    e_tau = np.max(np.abs(res['tau'] - tau) * Cm[:, 0] / (2.0 * dt * n_lags))
    print('max |dCt_vec| = %.3g, max |d dCt_vec| = %.3g, max |dtau| C_m(0) / (2 dt n_lags) = %.3g' % (e_ct, e_dct, e_tau))
    assert np.all(Cm[:, 0] > 0)
    assert e_ct <= 1e-9 and e_dct <= 2e-9 and e_tau <= 1e-9
    assert np.max(np.abs(res['Cm'] - Cm)) <= 1e-9
    # without mode_ct the result is what it was
    plain = ired.calculate_iRED(files, dt=dt, window=1000.0, ctx=ctx)
    assert sorted(plain) == ['M', 'S2', 'S2_w', 'dS2', 'eig', 'lam_w', 'win_len', 'win_start']
    for k in plain:
        assert plain[k].tobytes() == res[k].tobytes(), k


def test_cli_iRED_Ct(tmp_path):
    v = make_vectors(24, 1536)
    fn = str(tmp_path / 'vecs.npy')
    np.save(fn, v)
    script = os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')
    common = ['-s', 'none.pdb', '-f', fn, '--dt', '10', '--tau', '1280', '--binary', '--iRED', '--iRED_window', '3840']
    outs = []
    for name, extra in (('plain', []), ('modes', ['--iRED_Ct'])):
        d = tmp_path / name
        d.mkdir()
        p = subprocess.run([sys.executable, script] + common + ['-o', str(d / 'o')] + extra, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()[-3000:]
        outs.append(d)
    plain, modes = (sorted(os.listdir(str(d))) for d in outs)
    new = ['o_iRED_Ctint.dat', 'o_iRED_modeCt.dat', 'o_iRED_tau.dat']
    assert plain == ['o_iRED_S2.dat', 'o_iRED_eig.dat', 'o_iRED_matrix.npz'] and sorted(plain + new) == modes
    for f in ('o_iRED_S2.dat', 'o_iRED_eig.dat'):
        assert filecmp.cmp(str(outs[0] / f), str(outs[1] / f), shallow=False), f
    za, zb = (np.load(str(d / 'o_iRED_matrix.npz')) for d in outs)
    assert sorted(za.files) == ['M', 'resid', 'win_len', 'win_start']
    assert sorted(zb.files) == ['Cm_w', 'M', 'modes_w', 'resid', 'win_len', 'win_start']
    assert za['M'].tobytes() == zb['M'].tobytes()
    # the per-vector file against the library call at the precision the writer prints (numpy's str of a float64 array: eight
    # decimals in positional notation, eight digits behind the point of the mantissa in scientific): half a unit of the last one
    printed = dict(rtol=0.5e-8, atol=0.5e-8)
    with hip.Context() as c:
        res = ired.calculate_iRED([v], dt=10.0, window=3840.0, ctx=c, mode_ct=True)
    assert zb['Cm_w'].tobytes() == res['Cm_w'].tobytes() and zb['modes_w'].tobytes() == res['modes_w'].tobytes()
    legs, x, y, dy = gs.load_sxydylist(str(outs[1] / 'o_iRED_Ctint.dat'))
    assert [int(s) for s in legs] == list(range(2, 26))
    x, y, dy = np.array(x), np.array(y), np.array(dy)
    assert x.shape == y.shape == dy.shape == (24, 192)                    # lags 1 .. F_w // 2 of windows of 384 frames
    assert np.array_equal(x[0], np.arange(1, 193) * 10.0)
    assert np.allclose(y, res['Ct_vec'][1:].T, **printed) and np.allclose(dy, res['dCt_vec'][1:].T, **printed)
    legs, x, y, dy = gs.load_sxydylist(str(outs[1] / 'o_iRED_modeCt.dat'))
    assert [int(s) for s in legs] == list(range(1, 25)) and np.array(y).shape == (24, 193) and np.array(x)[0][0] == 0.0
    assert np.allclose(np.array(y), res['Cm'], **printed)
    tau = np.loadtxt(str(outs[1] / 'o_iRED_tau.dat'), comments='&')
    # print_xylist writes %g, six significant digits: half a unit of the sixth is at most 5e-6 of the value (mantissa 1.00000)
    assert tau.shape == (24, 3)
    assert np.allclose(tau[:, 1], res['eig'], rtol=5e-6, atol=0.0) and np.allclose(tau[:, 2], res['tau'], rtol=5e-6, atol=0.0)
