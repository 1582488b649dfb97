"""
GPU tests (marker gpu) of the distance-weighted dipolar correlation function of flexible spin pairs: k_dipolar_rmin, k_pack_dipolar,
k_ct_dipolar and k_ct_dipolar_norm (csrc/sr_ct_dipolar.hip) through the _dev entry points, hip.ResidentVectors.ct_dipolar,
spinrelax_amd.ct.calculate_Ct_dipolar* and the --dipolarCt flag of scripts/calculate-Ct-from-traj.py.

The oracle is the definition in float64 numpy (oracle_core / oracle_dipolar below), chunk-pooled like the library: per chunk
c_r(k) = [1.5 sum (a . a')^2 - 0.5 sum w w'] / (F - k) and n_r = sum w^2 / F, C = mean c_r / mean n_r, dC = std c_r / (sqrt(R) - 1) / mean n_r.
Bars:
  * the pack: 1e-7 absolute on a and w (they lie in [-1, 1]; half a float32 ulp there is 3e-8), 1e-14 relative on r_ref;
  * mode 1 (float64 throughout) against the definition on the planes the pack wrote: 1e-12 absolute on C and dC, 1e-12 relative on
    <w> and <w^2> -- float64 sums of at most 1000 terms in [0, 1] taken in another order differ by about 1e-13;
  * mode 0 (float32 products) against the definition on the raw vectors: the bars of the float32 direct-kernel size cases of
    tests/test_gpu_parity.py, quoted: relerr(C, Cr) < 1e-6 and dct_close; reff6, reff3 and S2rad 1e-6 relative.
The test vectors wobble by about 0.15 rad around axes within 15 degrees of z (the generator of tests/test_gpu_ct_cross.py) and their
distance is r0 exp(y), r0 in 0.18 .. 0.48, y an AR(1) process of standard deviation 0.1 and coefficient 0.9: C_dd stays above 0.66 at
every size here, so the relative bar means something.
"""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr
from test_gpu_ct_cross import dct_close, make_vectors
from spinrelax_amd import ct as hostct
from spinrelax_amd import general_scripts as gs
from spinrelax_amd.hip import SpinRelaxHipError

pytestmark = pytest.mark.gpu

V = 7
RTOL = 1e-6
SIZES = [(F, R) for F in (2, 3, 17, 128, 257, 1000) for R in (1, 3)]
# F <= 128: the float64 path alone; 257 and 1000: one-wave slabs (1000: with a tail of lags behind the last full block); 4096 and 4100:
# the four-wave workgroup with 16 lag blocks, 4100 with three lags behind them
SIZES32 = [(F, R, V) for F, R in SIZES] + [(4096, 2, 3), (4100, 2, 3)]


def make_pairs(N, seed, nV=V):
    """unit vectors u (N, nV, 3) float32, distances r (N, nV) float32 and the raw vectors float32(u r)"""
    u = make_vectors(N, seed, nV)
    rng = np.random.default_rng(seed + 7919)
    r0 = 0.18 + 0.30 * rng.random(nV)
    y = np.empty((N, nV))
    x = 0.1 * rng.standard_normal(nV)
    for t in range(N):
        x = 0.9 * x + 0.1 * np.sqrt(1 - 0.9 ** 2) * rng.standard_normal(nV)
        y[t] = x
    r = (r0[None] * np.exp(y)).astype(np.float32)
    raw = (u.astype(np.float64) * r.astype(np.float64)[..., None]).astype(np.float32)
    return u, r, raw


def planes_of(vec, dist=None):
    """The float64 expression of the pack: vec (N, V, 3), dist (N, V) or None -> a (N, V, 3), w (N, V), r_ref (V)"""
    v = np.asarray(vec, dtype=np.float64)
    ln = np.sqrt((v * v).sum(-1))
    r = ln if dist is None else np.asarray(dist, dtype=np.float64)
    rref = r.min(axis=0)
    w = (rref[None] / r) ** 3
    return v * (np.sqrt(w) / ln)[..., None], w, rref


def oracle_core(a4, w4, lags=None):
    """a4 (R, F, V, 3), w4 (R, F, V) -> C, dC (L or len(lags), V), <w>, <w^2> (V): the definition, float64"""
    a4, w4 = np.asarray(a4, dtype=np.float64), np.asarray(w4, dtype=np.float64)
    R, F = w4.shape[:2]
    ks = np.arange(1, F // 2 + 1) if lags is None else np.asarray(lags)
    c = np.empty((len(ks), R, w4.shape[2]))
    for m, k in enumerate(ks):
        Sa = (np.einsum('rtvc,rtvc->rtv', a4[:, :F - k], a4[:, k:]) ** 2).sum(axis=1)
        Sw = (w4[:, :F - k] * w4[:, k:]).sum(axis=1)
        c[m] = (1.5 * Sa - 0.5 * Sw) / (F - k)
    n = ((w4 ** 2).sum(axis=1) / F).mean(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        dC = np.std(c, axis=1) / (np.sqrt(R) - 1.0) / n
    return c.mean(axis=1) / n, dC, w4.mean(axis=(0, 1)), (w4 ** 2).mean(axis=(0, 1))


def oracle_dipolar(vec, dist, R, F, starts=None, lags=None):
    """vec (N, V, 3), dist (N, V) or None, chunks of F frames at `starts` (default r F) -> C, dC, reff6, reff3, S2rad"""
    a, w, rref = planes_of(vec, dist)
    starts = np.arange(R) * F if starts is None else starts
    a4 = np.stack([a[s:s + F] for s in starts])
    w4 = np.stack([w[s:s + F] for s in starts])
    C, dC, w1, w2 = oracle_core(a4, w4, lags)
    return C, dC, rref * w2 ** (-1.0 / 6.0), rref * w1 ** (-1.0 / 3.0), w1 * w1 / w2


@pytest.fixture(scope='module')
def ctx():
    from spinrelax_amd.hip import Context
    c = Context(0)
    yield c
    c.close()


_cache = {}


def case(F, R, nV=V):
    """(u, r, raw) of one size case and the oracle of the raw vectors, computed once"""
    if (F, R, nV) not in _cache:
        u, r, raw = make_pairs(R * F, seed=4000 + 10 * F + R, nV=nV)
        _cache[(F, R, nV)] = (u, r, raw, oracle_dipolar(raw, None, R, F))
    return _cache[(F, R, nV)]


def dev_pack(ctx, vec, dist, v0=0, nV=None):
    """sr_pack_dipolar_f32_dev on device copies: planes (nV, 4, Npad) float32 and r_ref (nV), downloaded, and the device planes"""
    import torch
    N, Vtot = vec.shape[:2]
    nV = Vtot - v0 if nV is None else nV
    Npad = (N + 63) // 64 * 64
    dv = torch.from_numpy(np.ascontiguousarray(vec, dtype=np.float32)).cuda()
    dd = None if dist is None else torch.from_numpy(np.ascontiguousarray(dist, dtype=np.float32)).cuda()
    planes = torch.full((nV, 4, Npad), 7.0, device='cuda', dtype=torch.float32)
    rref = torch.empty((nV,), device='cuda', dtype=torch.float64)
    ctx.pack_dipolar_dev(dv.data_ptr(), None if dd is None else dd.data_ptr(), N, Vtot, v0, nV, planes.data_ptr(), Npad, rref.data_ptr())
    ctx.sync()
    return planes.cpu().numpy(), rref.cpu().numpy(), planes, Npad


def dev_ct(ctx, planes, Npad, nV, R, F, mode):
    import torch
    L = F // 2
    Ct = torch.empty((L, nV), device='cuda', dtype=torch.float64)
    dCt = torch.empty((L, nV), device='cuda', dtype=torch.float64)
    wm = torch.empty((nV, 2), device='cuda', dtype=torch.float64)
    ctx.ct_dipolar_dev(planes.data_ptr(), Npad, nV, R, F, Ct.data_ptr(), dCt.data_ptr(), wm.data_ptr(), mode=mode)
    ctx.sync()
    return Ct.cpu().numpy(), dCt.cpu().numpy(), wm.cpu().numpy()


def test_pack(ctx):
    """both input forms, a column range of a wider array, a frame count that is no multiple of the tile"""
    N = 200
    u, r, raw = make_pairs(N, seed=11, nV=9)
    for vec, dist in ((raw, None), (u, r)):
        p, rref, _, Npad = dev_pack(ctx, vec, dist, v0=1, nV=7)
        a, w, rr = planes_of(vec[:, 1:8], None if dist is None else dist[:, 1:8])
        assert Npad == 256 and p.shape == (7, 4, 256)
        print('pack: |da| %.2e |dw| %.2e r_ref %.2e' % (np.max(np.abs(p[:, :3, :N] - a.transpose(1, 2, 0))), np.max(np.abs(p[:, 3, :N] - w.T)),
                                                         relerr(rref, rr)))
        assert np.max(np.abs(p[:, :3, :N] - a.transpose(1, 2, 0))) <= 1e-7
        assert np.max(np.abs(p[:, 3, :N] - w.T)) <= 1e-7
        assert relerr(rref, rr) <= 1e-14
        assert np.all(p[:, :, N:] == 0.0)
        assert np.max(p[:, 3]) == 1.0                                  # the frame of r_ref itself has w = 1


@pytest.mark.parametrize('F,R', SIZES)
def test_float64_mode_against_the_definition_on_the_planes(ctx, F, R):
    u, r, raw, _ = case(F, R)
    p, rref, planes, Npad = dev_pack(ctx, raw, None)
    C, dC, wm = dev_ct(ctx, planes, Npad, V, R, F, 1)
    a4 = p[:, :3, :R * F].transpose(2, 0, 1).reshape(R, F, V, 3)
    w4 = p[:, 3, :R * F].T.reshape(R, F, V)
    Cr, dCr, w1, w2 = oracle_core(a4, w4)
    assert C.shape == dC.shape == (F // 2, V)
    print('F=%d R=%d: |dC| %.2e <w> %.2e <w^2> %.2e' % (F, R, np.max(np.abs(C - Cr)), relerr(wm[:, 0], w1), relerr(wm[:, 1], w2)))
    assert np.max(np.abs(C - Cr)) <= 1e-12
    assert relerr(wm[:, 0], w1) <= 1e-12 and relerr(wm[:, 1], w2) <= 1e-12
    if R == 1:
        # the reference's std / (sqrt(R) - 1) at R = 1, whatever it gives: the same as C(t)'s own
        _, dCp = hostct.calculate_Ct_Palmer(u.reshape(R, F, V, 3), ctx=ctx, mode=1)
        np.testing.assert_array_equal(dC, dCp)
    else:
        assert np.max(np.abs(dC - dCr)) <= 1e-12


@pytest.mark.parametrize('F,R,nV', SIZES32)
def test_float32_mode_against_the_definition(ctx, F, R, nV):
    u, r, raw, ref = case(F, R, nV)
    Cr, dCr = ref[:2]
    assert Cr.min() >= 0.66
    got = hostct.calculate_Ct_dipolar(raw.reshape(R, F, nV, 3), ctx=ctx, mode=0)
    C, dC = got[:2]
    print('F=%d R=%d: min C %.3f relerr C %.2e reff6 %.2e reff3 %.2e S2rad %.2e' % (F, R, Cr.min(), relerr(C, Cr), relerr(got[2], ref[2]),
                                                                                    relerr(got[3], ref[3]), relerr(got[4], ref[4])))
    assert C.shape == dC.shape == (F // 2, nV)
    assert relerr(C, Cr) < RTOL
    if R == 1:
        assert np.all(np.isnan(dC)) and np.all(np.isnan(dCr))
    else:
        assert dct_close(dC, dCr, R, F)
    for g, w in zip(got[2:], ref[2:]):
        assert relerr(g, w) < RTOL
    again = hostct.calculate_Ct_dipolar(raw.reshape(R, F, nV, 3), ctx=ctx, mode=0)
    for g, w in zip(got, again):
        assert g.tobytes() == w.tobytes()                              # two runs: the same bytes
    if F == 257:
        # the other input form: unit vectors and the distances beside them
        alt = hostct.calculate_Ct_dipolar(u.reshape(R, F, nV, 3), dist=r.reshape(R, F, nV), ctx=ctx, mode=0)
        refd = oracle_dipolar(u, r, R, F)
        assert relerr(alt[0], refd[0]) < RTOL and (R == 1 or dct_close(alt[1], refd[1], R, F))
        for g, w in zip(alt[2:], refd[2:]):
            assert relerr(g, w) < RTOL


def test_limits(ctx):
    """the longest chunk whose four series fit the LDS, at 16 probed lags; one frame more is refused before anything runs"""
    F = ctx.ct_dipolar_max_frames()
    assert F == 10016                                                  # 16 bytes per frame and the padding, in 160 KiB
    L = F // 2
    lags = np.unique(np.linspace(1, L, 16).astype(int))
    assert len(lags) == 16
    u, r, raw = make_pairs(F + 1, seed=9, nV=1)
    with ctx.vectors(1, F + 1) as rv:
        rv.append(raw)
        C, dC, reff6, reff3, S2rad = hostct.calculate_Ct_dipolar_resident(rv, 1, F, mode=0)
        ref = oracle_dipolar(raw, None, 1, F, lags=lags)
        print('F=%d: relerr at the probed lags %.2e' % (F, relerr(C[lags - 1], ref[0])))
        assert relerr(C[lags - 1], ref[0]) < RTOL and relerr(reff6, ref[2]) < RTOL
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_dipolar(1, F + 1)
        assert '(-4)' in str(exc.value) and '10016' in str(exc.value)


def exact_unit_vectors(N, seed):
    """unit vectors that the pack's float32(u / |u|) leaves as they are: the normalisation iterated; the few vectors that keep hopping
    between two roundings are replaced by the z axis"""
    u = make_vectors(N, seed)
    for _ in range(4):
        d = u.astype(np.float64)
        u = (d / np.sqrt((d * d).sum(-1))[..., None]).astype(np.float32)
    d = u.astype(np.float64)
    n = (d / np.sqrt((d * d).sum(-1))[..., None]).astype(np.float32)
    hop = np.any(n != u, axis=-1)
    assert hop.mean() < 0.2
    u[hop] = (0.0, 0.0, 1.0)
    return u


@pytest.mark.parametrize('F,R', [(257, 3), (1000, 3)])
def test_constant_distance_is_the_autocorrelation(ctx, F, R):
    """unit vectors at a constant distance d (given beside them): w = 1 and a = u, bit for bit, so C_dd is C(t)"""
    d = np.float32(0.37)
    u = exact_unit_vectors(R * F, seed=31 + F)
    v4 = u.reshape(R, F, V, 3)
    dist = np.full((R, F, V), d, dtype=np.float32)
    for mode in (0, 1):
        Cp, dCp = hostct.calculate_Ct_Palmer(v4, ctx=ctx, mode=mode)
        C, dC, reff6, reff3, S2rad = hostct.calculate_Ct_dipolar(v4, dist=dist, ctx=ctx, mode=mode)
        if mode == 1:
            assert np.max(np.abs(C - Cp)) <= 1e-12 and np.max(np.abs(dC - dCp)) <= 1e-12
        else:
            assert relerr(C, Cp) < RTOL and dct_close(dC, dCp, R, F)
        assert relerr(reff6, np.full(V, float(d))) <= 1e-7 and relerr(reff3, np.full(V, float(d))) <= 1e-7
        assert np.max(np.abs(S2rad - 1.0)) <= 1e-12


def test_known_answer_alternating_distance(ctx):
    """A fixed direction, the distance alternating r1, r2 frame by frame, F even: C(k) = 1 for even k and 2 w1 w2 / (w1^2 + w2^2) for
    odd k, S2rad = (w1 + w2)^2 / (2 (w1^2 + w2^2)).  r1 / r2 = 1 / 4: w2 = 1 / 64 and sqrt(w2) = 1 / 8 are float32 numbers, so the
    planes hold the exact a and w and mode 1 meets the analytic value to rounding of the sums."""
    R, F, r1, r2 = 3, 200, 0.25, 1.0
    v = np.zeros((R * F, 1, 3), dtype=np.float32)
    v[0::2, :, 2], v[1::2, :, 2] = r1, r2
    w1, w2 = 1.0, (r1 / r2) ** 3
    odd = 2 * w1 * w2 / (w1 * w1 + w2 * w2)
    want = np.where(np.arange(1, F // 2 + 1) % 2 == 0, 1.0, odd)[:, None]
    s2 = (w1 + w2) ** 2 / (2 * (w1 * w1 + w2 * w2))
    for mode in (0, 1):
        C, dC, reff6, reff3, S2rad = hostct.calculate_Ct_dipolar(v.reshape(R, F, 1, 3), ctx=ctx, mode=mode)
        print('mode %d: |dC| %.2e S2rad %.2e' % (mode, np.max(np.abs(C - want)), abs(S2rad[0] - s2)))
        if mode == 1:
            assert np.max(np.abs(C - want)) <= 1e-12 and abs(S2rad[0] - s2) <= 1e-12 and np.max(np.abs(dC)) <= 1e-12
        else:
            assert relerr(C, want) < RTOL and relerr(S2rad, [s2]) < RTOL
        assert relerr(reff6, [r1 * (0.5 * (w1 * w1 + w2 * w2)) ** (-1.0 / 6.0)]) < RTOL


def test_ragged_chunks(ctx):
    """a chunk table with gaps and unequal file tails against the oracle on the same windows; r_ref runs over all frames held"""
    F = 130
    u, r, raw = make_pairs(5 * F + 48 + 7, seed=5)
    starts = np.array([0, F + 3, 2 * F + 3, 3 * F + 41, 4 * F + 48], dtype=np.int64)
    with ctx.vectors(V, raw.shape[0]) as rv:
        rv.append(raw)
        for mode in (0, 1):
            got = hostct.calculate_Ct_dipolar_resident(rv, 5, F, mode=mode, chunk_start=starts)
            ref = oracle_dipolar(raw, None, 5, F, starts=starts)
            assert relerr(got[0], ref[0]) < RTOL and dct_close(got[1], ref[1], 5, F)
            for g, w in zip(got[2:], ref[2:]):
                assert relerr(g, w) < RTOL
        # the three planes of the other analyses live beside the four: C(t) of the same object, before and after, the same bytes
        a = rv.ct(5, F, chunk_start=starts)
        rv.ct_dipolar(5, F, chunk_start=starts)
        b = rv.ct(5, F, chunk_start=starts)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        bad = starts.copy()
        bad[4] = raw.shape[0] - F + 1
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_dipolar(5, F, chunk_start=bad)
        assert '(-3)' in str(exc.value)


def test_bad_input(ctx):
    """a zero-length vector has no direction and no finite weight: refused with -3, by name; so is a distance that is not positive"""
    u, r, raw = make_pairs(100, seed=3)
    raw[40, 2] = 0.0
    with ctx.vectors(V, 100) as rv:
        rv.append(raw)
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_dipolar(1, 100)
        assert '(-3)' in str(exc.value) and 'vector 2' in str(exc.value)
        r[7, 3] = -1.0
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_dipolar(1, 100, dist=r)
        assert '(-3)' in str(exc.value)


def run(script, *args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', script)] + [str(a) for a in args], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-3000:]


def check_dipolar_files(d, want, names, dt, tau):
    """<d>/o_dipolarCtint.dat and <d>/o_dipolarDist.dat against the API's arrays (the text keeps 8 digits)"""
    C, dC, reff6, reff3, S2rad = want
    legs, t, Cf, dCf = gs.load_sxydylist(str(d / 'o_dipolarCtint.dat'), 'legend')
    assert [int(x) for x in legs] == list(names)
    assert np.allclose(np.array(t)[0], hostct.calculate_dt(dt, tau))
    assert np.max(np.abs(np.array(Cf) - C.T)) < 1e-7 and np.max(np.abs(np.array(dCf) - dC.T)) < 1e-7
    with open(str(d / 'o_dipolarDist.dat')) as fp:
        assert fp.readline().rstrip('\n') == '# resid reff6 reff3 S2rad'
    tab = np.loadtxt(str(d / 'o_dipolarDist.dat'))
    assert np.array_equal(tab[:, 0], np.array(names))
    assert relerr(tab[:, 1], reff6) < 1e-7 and relerr(tab[:, 2], reff3) < 1e-7 and relerr(tab[:, 3], S2rad) < 1e-7


def test_cli_dipolarCt(tmp_path, ctx):
    """--dipolarCt on an .npz with vecs + dist and on one with xyz writes its two files, which agree with the API; --Ct beside it
    writes the bytes it writes alone"""
    F, R = 64, 3
    u, r, raw = make_pairs(R * F + 5, seed=21)
    names = np.arange(11, 11 + V)
    fn = str(tmp_path / 'pairs.npz')
    np.savez(fn, vecs=u, dist=r, names=names, dt=1.0)
    for name, extra in (('plain', []), ('dip', ['--dipolarCt'])):
        (tmp_path / name).mkdir()
        run('calculate-Ct-from-traj.py', '-s', 'none.pdb', '-f', fn, '--tau', F, '--Ct', '-o', str(tmp_path / name / 'o'), *extra)
    assert sorted(os.listdir(str(tmp_path / 'dip'))) == sorted(os.listdir(str(tmp_path / 'plain')) + ['o_dipolarCtint.dat', 'o_dipolarDist.dat'])
    for f in ('o_Ctint.dat', 'o_Ctext.dat'):
        assert filecmp.cmp(str(tmp_path / 'plain' / f), str(tmp_path / 'dip' / f), shallow=False)
    want = hostct.calculate_Ct_dipolar(u[:R * F].reshape(R, F, V, 3), dist=r[:R * F].reshape(R, F, V), ctx=ctx)
    check_dipolar_files(tmp_path / 'dip', want, names, np.float32(1.0), float(F))
    # coordinates: X atoms anywhere, H = X + the raw vector; directions from the front end, distances from the coordinates
    rng = np.random.default_rng(4)
    xyz = np.zeros((R * F + 5, 2 * V, 3), dtype=np.float32)
    xyz[:, 0::2] = rng.standard_normal((R * F + 5, V, 3)).astype(np.float32)
    xyz[:, 1::2] = xyz[:, 0::2] + raw
    iX, iH = np.arange(0, 2 * V, 2), np.arange(1, 2 * V, 2)
    fx = str(tmp_path / 'coords.npz')
    np.savez(fx, xyz=xyz, indexX=iX, indexH=iH, dt=1.0)
    (tmp_path / 'xyz').mkdir()
    run('calculate-Ct-from-traj.py', '-s', 'none.pdb', '-f', fx, '--tau', F, '-o', str(tmp_path / 'xyz' / 'o'), '--dipolarCt')
    assert sorted(os.listdir(str(tmp_path / 'xyz'))) == ['o_dipolarCtint.dat', 'o_dipolarDist.dat']
    unit = hostct.obtain_XHvecs(xyz, iX, iH, ctx=ctx, bSuppressPrint=True)
    x64 = xyz.astype(np.float64)
    dist = np.linalg.norm(x64[:, iH] - x64[:, iX], axis=-1).astype(np.float32)
    want = hostct.calculate_Ct_dipolar(unit[:R * F].reshape(R, F, V, 3), dist=dist[:R * F].reshape(R, F, V), ctx=ctx)
    check_dipolar_files(tmp_path / 'xyz', want, np.arange(2, V + 2), np.float32(1.0), float(F))
