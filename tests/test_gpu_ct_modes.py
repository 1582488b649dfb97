"""
GPU tests (marker gpu) of the mode-resolved bond-vector correlation function: k_pack_modes, k_ct_modes and k_ct_modes_finalize
(csrc/sr_ct_modes.hip) through the _dev entry points, hip.ResidentVectors.ct_modes, spinrelax_amd.ct.calculate_Ct_modes*, modes.py on
the GPU's sums and the --modeCt flags of scripts/calculate-Ct-from-traj.py.  Mobile vectors throughout (a random walk on the sphere plus
jumps between two sites, test_ct_modes_host.mobile_vectors), of lengths 0.5 .. 2.

The reference of the correlation kernel is the definition in float64 numpy (test_ct_modes_host.oracle_modes) on the planes DOWNLOADED
from the library, so its bars are the kernel's arithmetic alone.  With n = F - k terms t in a sum, A = sum|t| / n (oracle_modes: absH),
u53 = 2^-53 and u = 2^-24:

  mode 1 and every lag that mode 0 leaves to the float64 path (lags from 128 floor((L + 1) / 128) on):
      BAR1(k) = (n + 2) u53 A     the textbook bound of a length-n sum with its products and the division.
  mode 0, full lag blocks.  As built (dip_shift_block_w, sr_ct_dipolar.h, with center = 0): a lane holds 4 accumulators per lag; a
      step adds two terms to each by v_fma_f32 (the product is not rounded by itself: one rounding per fma), kFlush = 8 steps between
      folds: at most 16 fmas per accumulator, so a term passes at most 16 roundings there, each relative to a partial sum that is at
      most sum|t| of the accumulator.  The fold (a0 + a1) + (a2 + a3) adds 2 roundings.  The conversion to float64 is exact, and the
      float64 additions of the folds, the strips and the chunks are inside BAR1.  First order: 18 u sum|t|; all orders:
      g18 = 18 u / (1 - 18 u).
      BAR0(k) = g18 A + BAR1(k).      H2 = (S01 + S10) / 2: A is the half sum of the two sums of |t|, the halving is exact.
  dH: the std over the chunks moves by at most the largest error of a chunk value: BAR(k) with A the largest over the chunks
      (absH_max), over sqrt(R) - 1, plus 4 u53 dH for its own arithmetic.
  smean: a float64 sum of R F terms: (R F + 2) u53 mean|s|.
The pack: each plane value is the float64 signal rounded once to float32: u |s|, plus 16 u53 for the float64 arithmetic in front of
the rounding (a dozen operations on values of at most 1).
"""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

import ct_inputs as ci
from conftest import ROOT
from test_ct_modes_host import FRAME, TENSORS, mobile_vectors, oracle_modes, signals
from spinrelax_amd import ct as hostct
from spinrelax_amd import modes, noe
from spinrelax_amd.hip import SpinRelaxHipError

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
U53 = 2.0 ** -53
G18 = 18 * U / (1 - 18 * U)
IDENT = np.array([2.25, 0.75, 0.0, 3.0, 3.0, 3.0])
FRAMES = [None, FRAME]


@pytest.fixture(scope='module')
def ctx():
    from spinrelax_amd.hip import Context
    c = Context(0)
    yield c
    c.close()


def make_raw(N, nV, seed):
    """mobile vectors of lengths 0.5 .. 2 as float32 (N, nV, 3), and the float32 unit vectors of the same directions"""
    u = mobile_vectors(N, nV, seed)
    ln = 0.5 + 1.5 * np.random.default_rng(seed + 1).random((N, nV))
    unit = u.astype(np.float32)
    unit = unit / np.linalg.norm(unit, axis=-1, keepdims=True).astype(np.float32)
    return (u * ln[..., None]).astype(np.float32), unit


def dev_pack(ctx, vec, frame=None, v0=0, nV=None):
    """sr_pack_modes_f32_dev on a device copy: planes (nV, 5, Npad) float32 and bad (nV), downloaded, and the device planes"""
    import torch
    N, Vtot = vec.shape[:2]
    nV = Vtot - v0 if nV is None else nV
    Npad = (N + 63) // 64 * 64
    dv = torch.from_numpy(np.ascontiguousarray(vec, dtype=np.float32)).cuda()
    planes = torch.full((nV, 5, Npad), 7.0, device='cuda', dtype=torch.float32)
    bad = torch.full((nV,), 9, device='cuda', dtype=torch.int32)
    ctx.pack_modes_dev(dv.data_ptr(), N, Vtot, v0, nV, planes.data_ptr(), Npad, bad.data_ptr(), frame=frame)
    ctx.sync()
    return planes.cpu().numpy(), bad.cpu().numpy(), planes, Npad


def dev_ct(ctx, planes, Npad, nV, R, F, mode, chunk_start=None):
    import torch
    L1 = F // 2 + 1
    H = torch.empty((L1, nV, 6), device='cuda', dtype=torch.float64)
    dH = torch.empty((L1, nV, 6), device='cuda', dtype=torch.float64)
    sm = torch.empty((nV, 5), device='cuda', dtype=torch.float64)
    ctx.ct_modes_dev(planes.data_ptr(), Npad, nV, R, F, H.data_ptr(), dH.data_ptr(), sm.data_ptr(), chunk_start=chunk_start, mode=mode)
    ctx.sync()
    return H.cpu().numpy(), dH.cpu().numpy(), sm.cpu().numpy()


def bars(ref, R, F, mode):
    """BAR for H and for dH, (L + 1, V, 6), by the module docstring"""
    L = F // 2
    n = (F - np.arange(L + 1))[:, None, None].astype(np.float64)
    fast = np.arange(L + 1) < ((L + 1) // 128) * 128 if mode == 0 else np.zeros(L + 1, dtype=bool)
    c = (n + 2) * U53 + np.where(fast, G18, 0.0)[:, None, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        return c * ref['absH'], c * ref['absH_max'] / (np.sqrt(R) - 1.0) + 4 * U53 * ref['dH']


def check_ct(tag, got, ref, R, F, mode):
    H, dH, sm = got
    bH, bdH = bars(ref, R, F, mode)
    L = F // 2
    assert H.shape == dH.shape == (L + 1, ref['H'].shape[1], 6)
    ratio = np.max(np.abs(H - ref['H']) / bH)
    bs = (R * F + 2) * U53 * ref['abs_s']
    rs = np.max(np.abs(sm - ref['smean']) / bs)
    print('%s F=%d R=%d mode %d: largest |dH| / bar %.3f, smean %.1e' % (tag, F, R, mode, ratio, rs), end='')
    assert ratio <= 1.0
    assert rs <= 1.0
    if R > 1:
        rd = np.max(np.abs(dH - ref['dH']) / bdH)
        print(', dH %.3f' % rd)
        assert rd <= 1.0
    else:
        print()
    return ratio


def reference(p, starts, F):
    """oracle_modes of the chunks at `starts` of the downloaded planes p (nV, 5, Npad)"""
    s4 = np.stack([p[:, :, s:s + F].astype(np.float64).transpose(2, 0, 1) for s in starts])
    ref = oracle_modes(s4)
    ref['abs_s'] = np.abs(s4).mean(axis=(0, 1))
    return ref


# ---- the pack ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nV', [1, 3, 33])
@pytest.mark.parametrize('frame', FRAMES, ids=['noframe', 'frame'])
def test_pack(ctx, nV, frame):
    """nV = 33 crosses the 32-vector tile edge, N = 67 the 64-frame one; a column range of a wider array"""
    N = 67
    raw, _ = make_raw(N, nV + 2, seed=100 + nV)
    p, bad, _, Npad = dev_pack(ctx, raw, frame, v0=1, nV=nV)
    v = raw[:, 1:1 + nV].astype(np.float64)
    ur = (v / np.linalg.norm(v, axis=-1, keepdims=True)) @ noe.frame_matrix(frame).T
    s = signals(ur).transpose(1, 2, 0)                      # (nV, 5, N)
    assert Npad == 128 and p.shape == (nV, 5, 128)
    ratio = np.max(np.abs(p[:, :, :N] - s) / (U * np.abs(s) + 16 * U53))
    print('pack nV=%d: largest |ds| / bar %.3f' % (nV, ratio))
    assert ratio <= 1.0
    assert np.all(p[:, :, N:] == 0.0)
    assert np.all(bad == 0)


def test_pack_and_entry_refusals(ctx):
    """a NaN frame and a zero vector are reported by the vector's name; a quaternion of norm 1.01 is refused before anything is
    queued; the context works afterwards"""
    import torch
    raw, _ = make_raw(70, 4, seed=7)
    for v, frame_no, value in ((2, 13, np.nan), (1, 66, 0.0)):
        x = raw.copy()
        x[frame_no, v] = value
        _, bad, _, _ = dev_pack(ctx, x)
        assert list(bad) == [1 if k == v else 0 for k in range(4)]
        with ctx.vectors(4, 70) as rv:
            rv.append(x)
            with pytest.raises(SpinRelaxHipError) as exc:
                rv.ct_modes(1, 70)
            assert '(-3)' in str(exc.value) and 'vector %d ' % v in str(exc.value)
    q = np.array([1.01, 0.0, 0.0, 0.0])
    dv = torch.from_numpy(raw).cuda()
    planes = torch.zeros((4, 5, 128), device='cuda', dtype=torch.float32)
    bad = torch.zeros((4,), device='cuda', dtype=torch.int32)
    for frame in (q, np.array([np.nan, 0, 0, 1.0])):
        with pytest.raises(SpinRelaxHipError) as exc:
            ctx.pack_modes_dev(dv.data_ptr(), 70, 4, 0, 4, planes.data_ptr(), 128, bad.data_ptr(), frame=frame)
        assert '(-3)' in str(exc.value) and 'quaternion' in str(exc.value)
    with ctx.vectors(4, 70) as rv:
        rv.append(raw)
        with pytest.raises(SpinRelaxHipError):
            rv.ct_modes(1, 70, frame=q)
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_modes(2, 36)                               # more frames than held
        assert '(-3)' in str(exc.value)
        H, _, _ = rv.ct_modes(1, 70)
    assert np.all(np.isfinite(H))


# ---- the correlation kernel ----------------------------------------------------------------------------------------------------
_cache = {}


def case(ctx, R, F, nV=3, starts=None):
    """planes of one size case on the device and their oracle, made once"""
    key = (R, F, nV, None if starts is None else tuple(starts))
    if key not in _cache:
        N = R * F if starts is None else max(starts) + F + 3
        raw, unit = make_raw(N, nV, seed=5000 + 7 * F + R)
        p, bad, planes, Npad = dev_pack(ctx, raw, FRAME)
        assert not bad.any()
        st = np.arange(R) * F if starts is None else np.asarray(starts)
        _cache[key] = (planes, Npad, reference(p, st, F), raw, unit)
    return _cache[key]


# F = 9, 37: the float64 path alone; 300 with an irregular chunk table: one full lag block and a tail; 1000: one-wave slabs, three
# blocks and a tail
SHAPES = [(1, 9, None), (3, 37, None), (2, 1000, None), (3, 300, (5, 311, 700))]


@pytest.mark.parametrize('mode', [1, 0])
@pytest.mark.parametrize('R,F,starts', SHAPES)
def test_ct_against_the_definition_on_the_planes(ctx, R, F, starts, mode):
    planes, Npad, ref, _, _ = case(ctx, R, F, starts=starts)
    got = dev_ct(ctx, planes, Npad, 3, R, F, mode, chunk_start=starts)
    check_ct('ct', got, ref, R, F, mode)


@pytest.mark.parametrize('mode', [1, 0])
def test_ct_at_the_longest_chunk(ctx, mode):
    """one vector at F = ct_modes_max_frames(): the four-wave workgroup with 31 lag blocks and all the LDS there is; F + 1 is refused
    with -4 and the context stays usable"""
    F = ctx.ct_modes_max_frames()
    assert 7900 <= F <= 8000
    planes, Npad, ref, _, _ = case(ctx, 1, F, nV=1)
    got = dev_ct(ctx, planes, Npad, 1, 1, F, mode)
    check_ct('longest', got, ref, 1, F, mode)


def test_ct_refuses_a_longer_chunk(ctx):
    F = ctx.ct_modes_max_frames()
    raw, _ = make_raw(F + 1, 1, seed=3)
    with ctx.vectors(1, F + 1) as rv:
        rv.append(raw)
        with pytest.raises(SpinRelaxHipError) as exc:
            rv.ct_modes(1, F + 1)
        assert '(-4)' in str(exc.value)
        with pytest.raises(ValueError):
            hostct.calculate_Ct_modes_resident(rv, 1, F + 1)
        H, _, _ = rv.ct_modes(1, 64)
    assert np.all(np.isfinite(H))


def test_R1_gives_the_dH_kernel_1_gives_for_dC(ctx):
    planes, Npad, _, _, unit = case(ctx, 1, 9)
    _, dH, _ = dev_ct(ctx, planes, Npad, 3, 1, 9, 1)
    _, dC = hostct.calculate_Ct_Palmer(unit.reshape(1, 9, 3, 3), ctx=ctx, mode=1)
    np.testing.assert_array_equal(dH[1:], np.broadcast_to(dC[:, :, None], dH[1:].shape))


# ---- the identity with kernel 1 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [1, 0])
@pytest.mark.parametrize('frame', FRAMES, ids=['noframe', 'frame'])
def test_identity_with_kernel_1(ctx, frame, mode):
    """2.25 H0 + 0.75 H1 + 3 (H3 + H4 + H5) against calculate_Ct_Palmer (float64 mode: bar ct_inputs.BAR_F64) on the same float32 unit
    vectors and chunks.  The bar is the sum of the two kernels' bars and of what the inputs differ by: the planes are the signals
    rounded to float32 (2 u per product of two of them), and kernel 1 takes the float32 vectors as they are, whose squared length
    1 + e scales (u . u')^2 by at most (1 + e)^2, e measured on the input here"""
    R, F, V = 3, 300, 3
    _, unit = make_raw(R * F, V, seed=77)
    Cp, _ = hostct.calculate_Ct_Palmer(unit.reshape(R, F, V, 3), ctx=ctx, mode=1)
    res = hostct.calculate_Ct_modes(unit.reshape(R, F, V, 3), frame=frame, ctx=ctx, mode=mode)
    assert np.array_equal(res['lags'], np.arange(F // 2 + 1)) and res['frame'].shape == (4,)
    C = res['H'] @ IDENT
    p, _, _, _ = dev_pack(ctx, unit, frame)
    ref = reference(p, np.arange(R) * F, F)
    bH, _ = bars(ref, R, F, mode)
    e = np.max(np.abs((unit.astype(np.float64) ** 2).sum(-1) - 1.0))
    bar = bH @ IDENT + 2 * U * (ref['absH'] @ IDENT) + 1.5 * (2 * e + e * e) + ci.BAR_F64
    ratio = np.max(np.abs(C[1:] - Cp) / bar[1:])
    print('identity mode %d: largest |dC| / bar %.3f (bar about %.2e)' % (mode, ratio, bar.mean()))
    assert ratio <= 1.0
    assert np.max(np.abs(C[0] - 1.0) / bar[0]) <= 1.0


# ---- bits ------------------------------------------------------------------------------------------------------------------------
def test_bits(ctx):
    """the same call twice gives the same bytes; a vector alone and among three gives the same bytes"""
    R, F = 2, 1000
    planes, Npad, _, raw, _ = case(ctx, R, F)
    a = dev_ct(ctx, planes, Npad, 3, R, F, 0)
    b = dev_ct(ctx, planes, Npad, 3, R, F, 0)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    _, _, alone, Npad1 = dev_pack(ctx, raw, FRAME, v0=1, nV=1)
    c = dev_ct(ctx, alone, Npad1, 1, R, F, 0)
    for x, y in zip(a, c):
        assert np.ascontiguousarray(x[..., 1:2, :] if x.ndim == 3 else x[1:2]).tobytes() == y.tobytes()


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_relaxation_from_the_gpu_sums(ctx):
    """modes.relaxation(stop='end') fed with the GPU's H and smean against the same function fed with the oracle's.  The bar pushes
    BAR0 and the smean bar through the host formulas: a = M H and c = M Hp are linear with the matrix M of noe.mode_amplitudes, Hp is
    quadratic in smean, J is linear in a and c with the weights of pl_transform and g(E_m, w), R1 and R2 are positive combinations of
    J, and NOE - 1 = K N / R1 with N = 6 J4 - J2"""
    R, F, h = 2, 1000, 2.0
    planes, Npad, ref, _, _ = case(ctx, R, F)
    H, dH, sm = dev_ct(ctx, planes, Npad, 3, R, F, 0)
    got = dict(H=H, dH=dH, smean=sm)
    D = TENSORS[0]
    bH, _ = bars(ref, R, F, 0)
    bs = (R * F + 2) * U53 * ref['abs_s']
    M = np.abs(noe.mode_amplitudes(np.eye(6), D))                                        # (6, 5): |d a_m / d H_c|
    m = np.abs(ref['smean'])
    i, j = np.array([0, 1, 0, 2, 3, 4]), np.array([0, 1, 1, 2, 3, 4])
    bHp = m[:, i] * bs[:, j] + m[:, j] * bs[:, i] + bs[:, i] * bs[:, j]
    da, dc = bH @ M, bHp @ M                                                             # (L + 1, V, 5), (V, 5)
    want = modes.relaxation(ref, D, h, 600.0, stop='end')
    have = modes.relaxation(got, D, h, 600.0, stop='end')
    om = want['omega']
    E = modes.amplitudes(ref, D)[2]
    W = np.abs(modes.pl_transform(np.eye(F // 2 + 1)[:, :, None, None], h, (E[:, None] + 1j * om[None, :])[None]))   # (L + 1, 5, 5): lag, mode, omega
    dJ = np.einsum('kvm,kmw->vw', da, W) + np.einsum('vm,mw->vw', dc, W.sum(axis=0) + (E[:, None] / (E[:, None] ** 2 + om[None] ** 2)))
    ratio = np.max(np.abs(have['J'] - want['J']) / dJ)
    from test_ct_modes_host import constants
    _, fDD, fCSA, tf, gr = constants(600.0)
    d0, d1, d2, d3, d4 = (dJ[:, k] for k in range(5))
    dR1 = tf * fDD * (d2 + 3 * d1 + 6 * d4) + fCSA * tf * d1
    dR2 = tf * 0.5 * fDD * (4 * d0 + d2 + 3 * d1 + 6 * d4 + 6 * d3) + fCSA * tf / 6.0 * (4 * d0 + 3 * d1)
    N = 6 * want['J'][:, 4] - want['J'][:, 2]
    dNOE = abs(tf * gr * fDD) * ((6 * d4 + d2) / want['R1'] + np.abs(N) * dR1 / want['R1'] ** 2) * (1 + 2 * dR1 / want['R1'])
    print('end to end: J %.1e R1 %.1e R2 %.1e NOE %.1e of their bars (relative bars %.1e %.1e %.1e)'
          % (ratio, np.max(np.abs(have['R1'] - want['R1']) / dR1), np.max(np.abs(have['R2'] - want['R2']) / dR2),
             np.max(np.abs(have['NOE'] - want['NOE']) / dNOE), np.max(dR1 / want['R1']), np.max(dR2 / want['R2']), np.max(dNOE)))
    assert ratio <= 1.0
    assert np.all(np.abs(have['R1'] - want['R1']) <= dR1)
    assert np.all(np.abs(have['R2'] - want['R2']) <= dR2)
    assert np.all(np.abs(have['NOE'] - want['NOE']) <= dNOE)
    assert np.all(want['R1'] > 0) and np.all(want['R2'] > want['R1'])


def run(script, *args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', script)] + [str(a) for a in args], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert p.returncode == 0, p.stdout.decode()[-3000:]


def test_cli_modeCt(tmp_path, ctx):
    """--modeCt --modeD --modeField on a synthetic .npz: the three files appear, _modeRelax.dat parses and agrees with the API, and
    --Ct beside them writes the bytes it writes alone"""
    F, R, V = 64, 3, 4
    _, unit = make_raw(R * F + 5, V, seed=21)
    names = np.arange(11, 11 + V)
    fn = str(tmp_path / 'vecs.npz')
    np.savez(fn, vecs=unit, names=names, dt=2.0)
    quat = ' '.join('%.17g' % x for x in FRAME)
    for name, extra in (('plain', []), ('modes', ['--modeCt', '--modeD', '2e7 1.8 0.3', '--modeField', '600'])):
        (tmp_path / name).mkdir()
        run('calculate-Ct-from-traj.py', '-s', 'none.pdb', '-f', fn, '--tau', 2.0 * F, '--Ct', '--vecRot', quat, '-o', str(tmp_path / name / 'o'),
            *extra)
    new = ['o_modeCt.npz', 'o_modeAmp.dat', 'o_modeRelax.dat']
    assert sorted(os.listdir(str(tmp_path / 'modes'))) == sorted(os.listdir(str(tmp_path / 'plain')) + new)
    for f in os.listdir(str(tmp_path / 'plain')):
        assert filecmp.cmp(str(tmp_path / 'plain' / f), str(tmp_path / 'modes' / f), shallow=False), f
    res = hostct.calculate_Ct_modes(unit[:R * F].reshape(R, F, V, 3), frame=FRAME, ctx=ctx)
    z = np.load(str(tmp_path / 'modes' / 'o_modeCt.npz'))
    assert sorted(k for k in z.files if k != 'names') == ['H', 'dH', 'dt', 'frame', 'lags', 'smean']
    assert z['H'].tobytes() == res['H'].tobytes() and z['smean'].tobytes() == res['smean'].tobytes() and float(z['dt']) == 2.0
    from spinrelax_amd._hostmath import ellipsoid_from_iso
    D = np.array(ellipsoid_from_iso(2e7, 1.8, 0.3)) * 1e-12
    rel = modes.relaxation(res, D, 2.0, 600.0)
    tab = np.loadtxt(str(tmp_path / 'modes' / 'o_modeRelax.dat'))
    assert tab.shape == (V, 4) and np.array_equal(tab[:, 0], names)
    for k, key in enumerate(('R1', 'R2', 'NOE')):
        assert np.max(np.abs(tab[:, k + 1] / rel[key] - 1.0)) < 1e-7
    amp = np.loadtxt(str(tmp_path / 'modes' / 'o_modeAmp.dat'))
    a, c, _ = modes.amplitudes(res, D)
    assert amp.shape == (V, 12) and np.max(np.abs(amp[:, 1:6] - a[0])) < 1e-7 and np.max(np.abs(amp[:, 11] - c.sum(axis=1))) < 1e-7
