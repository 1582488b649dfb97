"""
GPU tests of NOESY under anisotropic tumbling: the mode-resolved lagged map (csrc/sr_noe.hip), the mode-resolved rate kernel
(k_noesy_rates_modes, csrc/sr_noesy.hip) and everything above them: hip.Context.noe_modes / noesy_rates_modes,
noe.dipolar_map(..., modes=True, frame=...), noesy.rate_matrix(..., D=...) and --noesyD of scripts/calculate-Ct-from-traj.py.

Oracle (in this file): the definition in float64 numpy on the same float32 coordinates and the same float64 quaternions:
d = x_j - x_i of the coordinates converted to float64, r = |d|, u = F R(q_t) d / r with F = R(q_F), and per block b and lag k

    H0 .. H5 = sum_t w [qz qz', dl dl', (qz dl' + dl qz') / 2, uy uz vy vz, ux uz vx vz, ux uy vx vy],      W = sum_t w,
    w = r(t)^-3 r(t + k)^-3, qz = uz^2 - 1/3, dl = ux^2 - uy^2 (primes: the frame t + k)

Inputs: make_body of tests/test_gpu_noe.py, scrambled as in tests/test_gpu_noe_lagged.py.

Bars, u = 2^-24, absolute on H per component, first order in u.
Mode 1 (float64 throughout): the sum-order argument of tests/test_gpu_noe_lagged.py, every term of magnitude <= w: BAR1 = 1e-12 W.
Mode 0 (float32 per pair, frame and lag), the sequence of csrc/sr_noe.hip; |u_a| <= 1:
  d'_a (the matrix F R(q) formed in float64, rounded to float32 once: its rows have unit length)     5u r absolute, ri 4.5u relative
                                                                                     (tests/test_gpu_noe_lagged.py)
  u_a = d'_a ri                                5u + 4.5u |u_a| + 1 rounding: 10.5u absolute; v_a likewise
  a0 = fma(uz, uz, -1/3), |a0| <= 2/3          2 |uz| 10.5u = 21u, the constant 0.34u, the fma 0.67u: 22.5u
  a1 = fma(ux, ux, -(uy uy)), |a1| <= 1        2 (|ux| + |uy|) 10.5u <= 29.7u, uy uy rounded: u, the fma: u: 32u
  c = uy uz (and xz, xy), |c| <= 1/2           (|uy| + |uz|) 10.5u <= 14.85u, 1 rounding 0.5u: 15.4u
  g3 = (g g) g, g = ri si                      32u relative (tests/test_gpu_noe_lagged.py)
  t0 = (a0 b0) g3                              2 * 22.5u * 2/3 + 0.45u = 30.5u; g3: 32u * 4/9 + 0.45u = 14.7u: 45.2u w
  t1 = (a1 b1) g3                              2 * 32u + u = 65u; g3: 32u + u = 33u: 98u w
  t2 = (0.5 fma(a0, b1, a1 b0)) g3             a1 b0: 32u * 2/3 + 22.5u + 0.67u = 44.5u; a0 b1 inside the fma 43.9u, the fma 1.34u: 89.8u,
                                               halved exactly: 44.9u, |.| <= 2/3; g3: 32u * 2/3 + 0.67u = 22u: 67u w
  t3, t4, t5 = ((c) (c')) g3                   2 * 15.4u / 2 + 0.25u = 15.7u; g3: 32u / 4 + 0.25u = 8.3u: 24u w
  float32 partial sums of at most 8 terms, 7 roundings, each <= u sum |term|: 7u times the largest |term| / w: 3.1u, 7u, 4.7u, 1.75u
  BAR0 = (50, 105, 72, 26, 26, 26) u W.  The worst values measured on the device are in docs/EXPERIMENTS.md.
The identity 2.25 H0 + 0.75 H1 + 3 (H3 + H4 + H5) = G of k_noe_lagged: both sides inside their own bars of the exact sum:
  mode 0: (2.25 * 50 + 0.75 * 105 + 3 * 78) u = 425.25u of W for the modes and 116u for G; mode 1: (2.25 + 0.75 + 9 + 1) 1e-12 W.
  At lag 0 against the map's r^-6 sums, W = the sum itself: 425.25u + 39u relative in mode 0, 13e-12 + 1e-12 in mode 1.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import noesy_oracle as orc
from conftest import ROOT
from noesy_oracle import U53
from spinrelax_amd import _hostmath as hm
from spinrelax_amd import hip, noe, noesy
from spinrelax_amd._lib import SpinRelaxHipError
from test_gpu_noe import MIN_DIST, make_body, rotmat
from test_gpu_noe_lagged import BAR0 as BAR0_G
from test_gpu_noe_lagged import LAGS_120, LAGS_RAGGED, RAGGED, scrambled
from test_noe_modes_host import rates_modes_numpy

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BAR1 = 1e-12
BAR0 = np.array([50.0, 105.0, 72.0, 26.0, 26.0, 26.0]) * U
IDENT = np.array([2.25, 0.75, 0.0, 3.0, 3.0, 3.0])
BAR_IDENT = {0: float(IDENT @ BAR0) + BAR0_G, 1: (IDENT.sum() + 1.0) * BAR1}
BAR_LAG0 = {0: float(IDENT @ BAR0) + 39 * U, 1: (IDENT.sum() + 1.0) * BAR1 + 1e-12}
Q_F = np.array([0.5, -0.1, 0.7, 0.3]) / np.linalg.norm([0.5, -0.1, 0.7, 0.3])       # a generic frame quaternion
Q_G = np.array([0.2, 0.9, -0.3, 0.1]) / np.linalg.norm([0.2, 0.9, -0.3, 0.1])       # another
D_RHOMBIC = np.array([0.8, 1.0, 1.5]) * 1e7


@pytest.fixture(scope='module')
def ctx():
    c = hip.Context()
    yield c
    c.close()


def oracle_H(xyz, index, quat, frame, blocks, lags, min_dist=MIN_DIST):
    """H (B, K, npairs, 6) and W (B, K, npairs) by the definition; asserts the minimum distance"""
    x = np.asarray(xyz[:, index], dtype=np.float64)
    iu, ju = np.triu_indices(len(index), k=1)
    d = x[:, ju] - x[:, iu]
    r = np.sqrt((d * d).sum(axis=-1))
    assert r.min() >= min_dist, 'oracle: a pair comes as close as %.3g' % r.min()
    dp = d if quat is None else np.einsum('tab,tpb->tpa', rotmat(np.asarray(quat, dtype=np.float64)), d)
    if frame is not None:
        dp = dp @ rotmat(np.asarray(frame, dtype=np.float64)[None])[0].T
    u = dp / r[..., None]
    f = np.stack((u[..., 2] ** 2 - 1.0 / 3.0, u[..., 0] ** 2 - u[..., 1] ** 2, u[..., 1] * u[..., 2], u[..., 0] * u[..., 2],
                  u[..., 0] * u[..., 1]), axis=-1)                   # qz, dl, yz, xz, xy per frame and pair
    w = r ** -3
    H = np.empty((len(blocks), len(lags), iu.size, 6))
    W = np.empty(H.shape[:3])
    for b, (s, n) in enumerate(blocks):
        for q, k in enumerate(lags):
            a, c = f[s:s + n - k], f[s + k:s + n]
            ww = w[s:s + n - k] * w[s + k:s + n]
            H[b, q, :, 0] = (ww * a[..., 0] * c[..., 0]).sum(axis=0)
            H[b, q, :, 1] = (ww * a[..., 1] * c[..., 1]).sum(axis=0)
            H[b, q, :, 2] = (ww * 0.5 * (a[..., 0] * c[..., 1] + a[..., 1] * c[..., 0])).sum(axis=0)
            for m in (2, 3, 4):
                H[b, q, :, m + 1] = (ww * a[..., m] * c[..., m]).sum(axis=0)
            W[b, q] = ww.sum(axis=0)
    return H, W


def check_H(tag, got, ref, W, bar):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    e = np.max(np.abs(got - ref) / W[..., None], axis=(0, 1, 2))
    print('%s: |H - oracle| / W per component: %s = %s u (bar %s u)' % (tag, ' '.join('%.2g' % v for v in e), np.round(e / U, 2),
                                                                       np.round(np.broadcast_to(bar, (6,)) / U, 1)))
    assert np.all(e <= bar), tag


CASES = [(True, None), (True, Q_F), (False, None), (False, Q_F)]           # (with quat, frame)


def run_case(ctx, P, F, blocks, lags, mode):
    big, index, quat = scrambled(P, F)
    bs, bl = [b[0] for b in blocks], [b[1] for b in blocks]
    for with_q, frame in CASES:
        q = quat if with_q else None
        ref, W = oracle_H(big, index, q, frame, blocks, lags)
        got = ctx.noe_modes(big, index, lags, quat=q, frame=frame, block_start=bs, block_len=bl, mode=mode)
        check_H('mode %d P=%d F=%d B=%d %s %s' % (mode, P, F, len(blocks), 'quat' if with_q else 'lab', 'frame' if frame is not None else 'no frame'),
                got, ref, W, BAR1 if mode else BAR0)


@pytest.mark.parametrize('mode', (0, 1))
@pytest.mark.parametrize('P', (2, 33, 65))
def test_against_the_oracle(ctx, P, mode):
    """P = 2 (one diagonal tile, one pair), 33 (a partial second tile), 65 (three tiles, the last of one atom); 120 frames as one block
    at the lags 0, 1, 3, 16, 17, 31 and as three ragged blocks at lags up to 19; with the quaternions and without, with a frame
    quaternion and without (all four instantiations and the identity-matrix path), the atoms a permuted subset of twice as many.
    Mode 0 is held to the first-order worst-case bound per component derived in this file's docstring."""
    run_case(ctx, P, 120, [(0, 120)], LAGS_120, mode)
    run_case(ctx, P, 120, RAGGED, LAGS_RAGGED, mode)


@functools.lru_cache(maxsize=None)
def split_case():
    P, F = 33, 1000
    _, xyz, quat = make_body(P, F)
    lags = (0, 5, 129, 700)
    ref, W = oracle_H(xyz, np.arange(P), quat, Q_F, [(0, F)], lags)
    return xyz, quat, lags, ref, W


@pytest.mark.parametrize('mode', (0, 1))
def test_frame_splits(ctx, mode):
    """P = 33, 1000 frames: seven frame splits (asserted > 1: otherwise the case is vacuous), partial tiles added by
    k_noe_finish; lag 129 reads frames of the next split, lag 700 leaves splits of 43 origins"""
    xyz, quat, lags, ref, W = split_case()
    assert ctx.noe_lagged_splits(33, 1000, 1) > 1
    got = ctx.noe_modes(xyz, np.arange(33), lags, quat=quat, frame=Q_F, mode=mode)
    check_H('mode %d, frame splits' % mode, got, ref, W, BAR1 if mode else BAR0)
    G = ctx.noe_lagged(xyz, np.arange(33), lags, quat=quat, mode=mode)
    e = np.max(np.abs(got @ IDENT - G) / W)
    print('mode %d, splits: identity %.3g (bar %.3g)' % (mode, e, BAR_IDENT[mode]))
    assert e <= BAR_IDENT[mode]


@pytest.mark.parametrize('mode', (0, 1))
def test_identity_with_the_lagged_map_in_any_frame(ctx, mode):
    """2.25 H0 + 0.75 H1 + 3 (H3 + H4 + H5) is ctx.noe_lagged's G on the same input, within the sum of both bars, whatever the frame
    quaternion; at lag 0 it is the map's r^-6 sum"""
    P, F = 33, 120
    _, xyz, quat = make_body(P, F)
    bs, bl = [b[0] for b in RAGGED], [b[1] for b in RAGGED]
    index = np.arange(P)
    G = ctx.noe_lagged(xyz, index, LAGS_RAGGED, quat=quat, block_start=bs, block_len=bl, mode=mode)
    sums = ctx.noe_pairs(xyz, index, quat=quat, block_start=bs, block_len=bl, mode=mode)
    _, W = oracle_H(xyz, index, quat, None, RAGGED, LAGS_RAGGED)
    combos = []
    for frame in (None, Q_F, Q_G):
        H = ctx.noe_modes(xyz, index, LAGS_RAGGED, quat=quat, frame=frame, block_start=bs, block_len=bl, mode=mode)
        combos.append(H @ IDENT)
        e = np.max(np.abs(combos[-1] - G) / W)
        e0 = np.max(np.abs(combos[-1][:, 0] / sums[:, :, 0] - 1))
        print('mode %d frame %s: identity %.3g (bar %.3g), lag 0 against the r^-6 sums %.3g (bar %.3g)' % (mode, frame, e, BAR_IDENT[mode], e0, BAR_LAG0[mode]))
        assert e <= BAR_IDENT[mode] and e0 <= BAR_LAG0[mode]
    # the frames against each other: each within its own bar of the same exact sum
    bar = 2 * (float(IDENT @ BAR0) if mode == 0 else IDENT.sum() * BAR1)
    assert np.max(np.abs(combos[1] - combos[0]) / W) <= bar and np.max(np.abs(combos[2] - combos[1]) / W) <= bar
    # and the sums themselves do depend on the frame
    Ha, Hb = ctx.noe_modes(xyz, index, [0], quat=quat, frame=Q_F, mode=mode), ctx.noe_modes(xyz, index, [0], quat=quat, mode=mode)
    assert np.max(np.abs(Ha - Hb)) > 1e-3 * np.max(np.abs(Hb))


def test_equal_bits_from_call_to_call_and_alone_or_in_a_list(ctx):
    """two calls give the same bits; a lag computed alone has the bits it has in a list -- also where the frames are split"""
    for P, F, blocks, lags in ((65, 120, RAGGED, LAGS_RAGGED), (33, 300, [(0, 300)], [0, 5, 64])):
        _, xyz, quat = make_body(P, F)
        bs, bl = [b[0] for b in blocks], [b[1] for b in blocks]
        for mode in (0, 1):
            kw = dict(quat=quat, frame=Q_F, block_start=bs, block_len=bl, mode=mode)
            a = ctx.noe_modes(xyz, np.arange(P), lags, **kw)
            b = ctx.noe_modes(xyz, np.arange(P), lags, **kw)
            assert np.isfinite(a).all() and a.tobytes() == b.tobytes()
            for q, k in enumerate(lags):
                one = ctx.noe_modes(xyz, np.arange(P), [k], **kw)
                assert one.shape == (len(bs), 1, noe.n_pairs(P), 6) and one[:, 0].tobytes() == a[:, q].tobytes(), (P, mode, k)
    assert ctx.noe_lagged_splits(33, 300, 1) > 1


def test_refusals_leave_the_context_usable(ctx):
    """host checks: nothing reaches the device with bad arguments, and the context gives the same bits afterwards"""
    _, xyz, quat = make_body(5, 17)
    good = ctx.noe_modes(xyz, np.arange(5), [0, 1, 5], quat=quat, frame=Q_F)

    def refused(pattern, bs=(0,), bl=(17,), lags=(0, 1, 5), frame=Q_F, mode=0, index=np.arange(5)):
        with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_noe_modes_check: .*' + pattern):
            ctx.noe_modes(xyz, index, list(lags), quat=quat, frame=frame, block_start=list(bs), block_len=list(bl), mode=mode)
        assert ctx.noe_modes(xyz, np.arange(5), [0, 1, 5], quat=quat, frame=Q_F).tobytes() == good.tobytes()

    refused('lag 17 leaves no term in a block of 17 frames', lags=(1, 17))
    refused('lag 8 leaves no term in a block of 8 frames', bs=(0, 9), bl=(9, 8), lags=(1, 8))
    refused(r'K=65 lags', lags=range(65))
    refused(r'K=0 lags', lags=())
    refused(r'strictly increasing: lag\[1\] = 2 after 4', lags=(4, 2))
    refused(r'lag\[0\] = -1 is negative', lags=(-1, 2))
    refused('not a unit quaternion', frame=[1.0, 0.1, 0.0, 0.0])
    refused('not a unit quaternion', frame=[0.0, 0.0, 0.0, 0.0])
    refused('component 2 = nan is not finite', frame=[1.0, 0.0, np.nan, 0.0])
    refused('component 0 = inf is not finite', frame=[np.inf, 0.0, 0.0, 0.0])
    refused('a pair needs two', index=[3])
    refused('mode 2', mode=2)
    with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_noe_modes_f32_dev: .*not a unit quaternion'):
        ctx.noe_modes_dev(0x1000, 17, 5, np.arange(5), None, [0], [17], [0, 1], 0x1000, frame=[2.0, 0.0, 0.0, 0.0])
    # 40000 atoms: the lagged map of 9 lags fits the device (58 GB), its six mode sums do not (346 GB)
    with pytest.raises(SpinRelaxHipError, match=r'9 lags x 799980000 pairs x 6 x 8 bytes = .* do not fit the device'):
        ctx.noe_modes_check(70, 40000, np.arange(40000), [0], [70], np.arange(9))
    ctx.noe_lagged_check(70, 40000, np.arange(40000), [0], [70], np.arange(9))
    assert ctx.noe_modes(xyz, np.arange(5), [0, 1, 5], quat=quat, frame=Q_F).tobytes() == good.tobytes()
    # through the module: the lags are refused before the map is computed (by the lagged map's check, which comes first)
    with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_noe_lagged_check: .*leaves no term'):
        noe.dipolar_map(xyz, np.arange(5), quat=quat, lags=[0, 20], modes=True, ctx=ctx)


# ---- the rate kernel ----
def mode_tables(P, seed=0):
    """a, c (npairs, 5) of the synthetic input of noesy_oracle, split at random over the modes, one mode rigid (a = c) and one empty"""
    A6, S2, _ = orc.synthetic(P)
    rng = np.random.default_rng(50 * P + seed)
    a = A6[:, None] * rng.dirichlet(np.ones(5), A6.size)
    c = a * rng.uniform(0.2, 0.95, a.shape)
    c[:, 1] = a[:, 1]
    a[::3, 4] = c[::3, 4] = 0.0
    return a, c


@pytest.mark.parametrize('te_kind', ('scalar', 'pair', 'mode'))
@pytest.mark.parametrize('P', (2, 47, 65))
def test_rates_modes_against_numpy(ctx, P, te_kind):
    """the bars of tests/test_gpu_noesy.py: J is now a sum of ten positive terms of some six float64 roundings each, still far inside
    64 u53 of the five-term magnitude; the diagonal adds the row sum's P u53 sum rho"""
    a, c = mode_tables(P)
    E = hm.D_coefficients_ellipsoid(D_RHOMBIC)
    rng = np.random.default_rng(P)
    n = a.shape[0]
    te = {'scalar': 5e-11, 'pair': rng.uniform(1e-12, 1e-9, n), 'mode': rng.uniform(1e-12, 1e-9, (n, 5))}[te_kind]
    leak = rng.uniform(0.0, 1.0, P)
    w = orc.omega_H(orc.FIELD)
    ref, RHO, MAG = rates_modes_numpy(a, c, E, P, w, te, leak, orc.Q_ANGSTROM)
    R = ctx.noesy_rates_modes(a, c, E, P, w, te, leak, orc.Q_ANGSTROM)
    off = ~np.eye(P, dtype=bool)
    print('P=%d tau_e %s: off-diagonal %.3g of 64 u53 MAG' % (P, te_kind, np.max(np.abs(R - ref)[off] / (64 * U53 * MAG[off]))))
    assert np.all(np.abs(R - ref)[off] <= 64 * U53 * MAG[off])
    assert np.all(np.abs(np.diagonal(R) - np.diagonal(ref)) <= P * U53 * RHO.sum(axis=1) + 64 * U53 * np.diagonal(ref))
    assert R.tobytes() == R.T.copy().tobytes()
    import torch
    R_d = torch.empty((P, P), dtype=torch.float64, device=torch.device('cuda', ctx.device))
    torch.cuda.synchronize()
    ctx.noesy_rates_modes_dev(a, c, E, P, w, te, leak, orc.Q_ANGSTROM, R_d.data_ptr())
    ctx.sync()
    assert R_d.cpu().numpy().tobytes() == R.tobytes()


def test_rate_modes_refusals_leave_the_context_usable(ctx):
    P = 5
    a, c = mode_tables(P)
    E = hm.D_coefficients_ellipsoid(D_RHOMBIC)
    w = orc.omega_H(600.0)
    good = ctx.noesy_rates_modes(a, c, E, P, w, 1e-10, 0.0, orc.Q_ANGSTROM)

    def again():
        return ctx.noesy_rates_modes(a, c, E, P, w, 1e-10, 0.0, orc.Q_ANGSTROM)

    def refused(pattern, a=a, c=c, E=E, P=P, te=1e-10, leak=0.0):
        with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_noesy_rates_modes_f64: .*' + pattern):
            ctx.noesy_rates_modes(a, c, E, P, w, te, leak, orc.Q_ANGSTROM)
        assert again().tobytes() == good.tobytes()          # nothing was queued: the context works, the same bits

    def with_(x, k, m, v):
        y = x.copy()
        y[k, m] = v
        return y
    refused('a pair needs two', a=a[:0], c=c[:0], P=1)
    refused(r'a\[3\]\[2\] = -', a=with_(a, 3, 2, -1e-3))
    refused(r'a\[3\]\[2\] = nan', a=with_(a, 3, 2, np.nan))
    refused(r'c\[0\]\[0\] = -', c=with_(c, 0, 0, -1e-9))
    refused(r'c\[2\]\[1\] = .* is above a', c=with_(c, 2, 1, a[2, 1] * (1 + 2e-6)))
    refused(r'E\[4\] = 0', E=np.concatenate([E[:4], [0.0]]))
    refused(r'E\[1\] = inf', E=np.array([E[0], np.inf, E[2], E[3], E[4]]))
    refused(r'tau_e = 0', te=0.0)
    refused(r'tau_e\[1\] = -', te=np.array([1e-10, -1e-10] + [1e-10] * 8))
    refused(r'tau_e\[9\]\[4\] = 0', te=with_(np.full((10, 5), 1e-10), 9, 4, 0.0))
    refused(r'leak = -1', leak=-1.0)
    refused(r'leak\[4\] = -', leak=np.array([0.0, 0.0, 0.0, 0.0, -0.5]))
    ok = ctx.noesy_rates_modes(a, with_(c, 2, 1, a[2, 1] * (1 + 5e-7)), E, P, w, 1e-10, 0.0, orc.Q_ANGSTROM)       # inside the tolerance
    assert np.isfinite(ok).all()


def test_map_with_modes_keeps_the_map_and_adds_the_sums(ctx):
    """dipolar_map(..., modes=True) holds, bit for bit, the map with the same lags, and H, H_blocks, frame by finalize_modes from the
    library's sums; lags=None means [0] and no lagged map; the superposed form reads the coordinates it uploaded once"""
    P, F = 33, 120
    body, xyz, quat = make_body(P, F)
    index = np.arange(P)
    blocks = ([0, 40, 80], [40, 40, 40])
    lags = [0, 1, 2, 4, 8]
    plain = noe.dipolar_map(xyz, index, quat=quat, blocks=blocks, ctx=ctx, lags=lags, dt=2.0)
    res = noe.dipolar_map(xyz, index, quat=quat, blocks=blocks, ctx=ctx, lags=lags, dt=2.0, modes=True, frame=Q_F)
    for k, v in plain.items():
        assert np.asarray(v).tobytes() == np.asarray(res[k]).tobytes(), k
    assert set(res) - set(plain) == {'H', 'H_blocks', 'frame'}
    Hb = ctx.noe_modes(xyz, index, lags, quat=quat, frame=Q_F, block_start=blocks[0], block_len=blocks[1])
    want = noe.finalize_modes(Hb, blocks[1], lags, Q_F)
    for k in ('H', 'H_blocks', 'frame'):
        assert np.asarray(res[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    assert res['H'].shape == (5, noe.n_pairs(P), 6)
    only = noe.dipolar_map(xyz, index, quat=quat, blocks=blocks, ctx=ctx, modes=True)
    assert only['lags'].tolist() == [0] and 'G' not in only and only['H'].shape == (1, noe.n_pairs(P), 6)
    assert only['H_blocks'].tobytes() == ctx.noe_modes(xyz, index, [0], quat=quat, block_start=blocks[0], block_len=blocks[1]).tobytes()
    sup = noe.dipolar_map_superposed(xyz, body.astype(np.float32), index, index, blocks=blocks, ctx=ctx, lags=lags, dt=2.0, modes=True, frame=Q_F)
    Hs = ctx.noe_modes(xyz, index, lags, quat=sup['quat'], frame=Q_F, block_start=blocks[0], block_len=blocks[1])
    assert sup['H_blocks'].tobytes() == Hs.tobytes() and sup['G'].shape == (3, 5, noe.n_pairs(P))


def test_isotropic_limit_on_a_real_map(ctx):
    """a, c of a real map in mode 1 and the sphere's tensor against ctx.noesy_rates on the same map's A6 and S2: both kernels inside
    their bars, and sum_m a_m = A6 up to the identity's bar at lag 0 (14e-12 relative, a factor on every rate; sum_m c_m = S2 A6 to
    float64 rounding)"""
    P = 33
    _, xyz, quat = make_body(P, 120)
    m = noe.dipolar_map(xyz, np.arange(P), quat=quat, mode=1, ctx=ctx, lags=[0, 1, 2, 4, 8, 16], dt=2e-12, modes=True, frame=Q_F)
    Diso = 1.0 / (6.0 * 5e-9)
    D = np.full(3, Diso)
    w = orc.omega_H(600.0)
    a, c, E = noesy.mode_inputs(m, D)
    assert np.max(np.abs(a.sum(axis=1) / m['A6'] - 1)) <= BAR_LAG0[1] and np.max(np.abs(c.sum(axis=1) / (m['S2'] * m['A6']) - 1)) <= 1e-13
    te = noesy.map_tau_e(m)
    R = noesy.rate_matrix(m, 600.0, D=D, tau_e='map', leak=0.3, ctx=ctx)
    R0 = noesy.rate_matrix(m, 600.0, 5e-9, tau_e='map', leak=0.3, ctx=ctx)
    assert R.tobytes() == ctx.noesy_rates_modes(a, c, E, P, w, te, 0.3, noesy.prefactor('nm')).tobytes()
    _, RHO, MAG = orc.rate_matrix(m['A6'], m['S2'], P, w, 5e-9, te, 0.3, orc.Q_NM)
    off = ~np.eye(P, dtype=bool)
    tol = 2 * 64 * U53 + BAR_LAG0[1]
    print('isotropic limit: off-diagonal %.3g of its bar' % np.max(np.abs(R - R0)[off] / (tol * MAG[off])))
    assert np.all(np.abs(R - R0)[off] <= tol * MAG[off])
    assert np.all(np.abs(np.diagonal(R) - np.diagonal(R0)) <= 2 * P * U53 * RHO.sum(axis=1) + tol * np.diagonal(R0))
    # per-mode tau_e: every mode of the sphere decays alike only if the motion is isotropic; it is a different matrix, still symmetric
    Rm = noesy.rate_matrix(m, 600.0, D=D_RHOMBIC, tau_e='modes', ctx=ctx)
    assert Rm.tobytes() == Rm.T.copy().tobytes() and np.isfinite(Rm).all()
    assert Rm.tobytes() == ctx.noesy_rates_modes(*noesy.mode_inputs(m, D_RHOMBIC)[:2], hm.D_coefficients_ellipsoid(D_RHOMBIC), P, w,
                                                 noesy.mode_tau_e(m, D_RHOMBIC), 0.0, noesy.prefactor('nm')).tobytes()
    out = noesy.noesy(m, [0.05, 0.2], 600.0, D=D_RHOMBIC, tau_e='modes', ctx=ctx)
    assert out['R'].tobytes() == Rm.tobytes() and out['A'].shape == (2, P, P)


def test_rigid_body_end_to_end(ctx):
    """A rigid body, tumbled, mode 1, the frame quaternion q_F, a rhombic tensor: every sigma_ij and rho_ij is q r^-6 [.] with
    J = _hostmath.J_combine_ellipsoid_exp_decayN(w, F d / r, D, 1, [], []) on the BUILT body, up to the float32 rounding of the
    coordinates (tests/test_gpu_noe.py, test_rigid_body_with_quaternions): distance and direction of a pair are off by at most
    rho = 2 sqrt(3) 2^-19 / r_min relative.  First order in rho: r^-6 moves by 6 rho; the amplitudes A_m(u) are quartics of the unit
    vector u with |grad 3 y^2 z^2| <= 3 (modes 0 .. 2), |grad dd| = 3 |(x^3, y^3, z^3)| <= 3 and |grad e| <= sum_i |c_i| (12 + 6) <= 9
    (|c_i| <= 1/6): sum_m |dA_m| <= (9 + 2 (3 + 9)) rho = 33 rho, so |dJ(w)| <= 33 rho max_m g(E_m, w).  With |J(w)| <= max_m g(E_m, w)
    = Gmax(w): |d sigma| <= 39 rho q r^-6 (6 Gmax(2w) + Gmax(0)), |d rho_ij| <= 39 rho q r^-6 (Gmax(0) + 3 Gmax(w) + 6 Gmax(2w)).  The
    internal term a_m - c_m of a rigid pair is second order in rho; the kernels' own 1e-12 is far below."""
    P, F = 33, 120
    body, xyz, quat = make_body(P, F, False)
    D = D_RHOMBIC
    w, q = orc.omega_H(600.0), noesy.prefactor('nm')
    E = hm.D_coefficients_ellipsoid(D)
    Fm = rotmat(Q_F[None])[0]

    def rates_of(u, r):
        Jw = hm.J_combine_ellipsoid_exp_decayN([0.0, w, 2 * w], u, D, 1.0, [], [])
        return q * r ** -6 * (6 * Jw[..., 2] - Jw[..., 0]), q * r ** -6 * (Jw[..., 0] + 3 * Jw[..., 1] + 6 * Jw[..., 2])
    # the test can see anisotropy: a pair along z against one along x, in the tensor's frame
    sz, sx = rates_of(np.array([0.0, 0.0, 1.0]), 0.3)[0], rates_of(np.array([1.0, 0.0, 0.0]), 0.3)[0]
    assert abs(sz / sx - 1) > 0.05
    iu, ju = np.triu_indices(P, k=1)
    d = body[ju] - body[iu]
    r = np.linalg.norm(d, axis=1)
    rho = 2 * np.sqrt(3.0) * 2.0 ** -19 / r.min()
    sig, rh = rates_of((d / r[:, None]) @ Fm.T, r)
    Gmax = [np.max(E / (E * E + om * om)) for om in (0.0, w, 2 * w)]
    m = noe.dipolar_map(xyz, np.arange(P), quat=quat, mode=1, ctx=ctx, modes=True, frame=Q_F)
    R = noesy.rate_matrix(m, 600.0, D=D, tau_e=1e-10, ctx=ctx)
    es = np.max(np.abs(R[iu, ju] - sig) / (q * r ** -6 * (6 * Gmax[2] + Gmax[0])))
    RHO = np.zeros((P, P))
    RHO[iu, ju] = RHO[ju, iu] = rh
    BND = np.zeros((P, P))
    BND[iu, ju] = BND[ju, iu] = q * r ** -6 * (Gmax[0] + 3 * Gmax[1] + 6 * Gmax[2])
    ed = np.max(np.abs(np.diagonal(R) - RHO.sum(axis=1)) / BND.sum(axis=1))
    print('rigid body: sigma %.3g, R_ii %.3g (bar 39 rho = %.3g)' % (es, ed, 39 * rho))
    assert es <= 39 * rho and ed <= 39 * rho
    # without the frame quaternion the rates are those of another orientation: the test sees the frame
    R_lab = noesy.rate_matrix(noe.dipolar_map(xyz, np.arange(P), quat=quat, mode=1, ctx=ctx, modes=True), 600.0, D=D, tau_e=1e-10, ctx=ctx)
    assert np.max(np.abs(R_lab[iu, ju] - sig) / (q * r ** -6 * (6 * Gmax[2] + Gmax[0]))) > 10 * 39 * rho


# ---- the command line ----
def run_cli(tmp_path, name, fn, extra):
    script = os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')
    d = tmp_path / name
    d.mkdir()
    p = subprocess.run([sys.executable, script, '-s', 'none.pdb', '-f', fn, '--tau', '500', '-o', str(d / 'o'), '--noeMap', '--binary', '--exact',
                        '--noesy', '--noesyMix', '0.05 0.2', '--noesyField', '600'] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    return d


def last_digit_apart(a, b):
    """two numbers printed as %.8g: at most one unit of the eighth significant digit apart"""
    x, y = float(a), float(b)
    if x == y:
        return True
    return abs(x - y) <= 1.0000001 * 10.0 ** (np.floor(np.log10(max(abs(x), abs(y)))) - 7)


def test_cli_noesyD(tmp_path, ctx):
    """--noesyD "D 1.0" (a sphere) against --noesyTauC 1 / (6 D): the columns of <o>_noesy.dat agree to the printed 8 digits, bar one
    unit in the last (--exact: in float32 the sum of the mode amplitudes is <r^-6> only to its float32 bar, which 8 digits would show);
    a rhombic run with --vecRot writes the file and H into the npz, the library called directly gives the same R; a run without
    --noesyD writes exactly the files it writes today, with no H"""
    P, F, nA = 12, 200, 20
    body, xyz, _ = make_body(nA, F)
    indexP = np.array([1, 4, 5, 7, 8, 10, 11, 13, 14, 16, 17, 19])
    fit = np.arange(nA)
    ref32 = body.astype(np.float32)
    fn = str(tmp_path / 'traj.npz')
    np.savez(fn, xyz=xyz, indexP=indexP, ref_xyz=ref32, fit_indices=fit, namesP=np.array(['H%d' % a for a in indexP]), dt=np.float32(10.0))
    lag_args = ['--noeLags', '1 2 4 8 16', '--noesyTauEMap']
    sph = run_cli(tmp_path, 'sph', fn, ['--noesyD', '%.17g 1.0' % (1.0 / (6.0 * 5e-9)), '--noesyTauE', '1e-10'])
    iso2 = run_cli(tmp_path, 'iso2', fn, ['--noesyTauC', '5e-9', '--noesyTauE', '1e-10'])
    assert sorted(os.listdir(str(iso2))) == ['o_noeMap.dat', 'o_noeMap.npz', 'o_noesy.dat', 'o_noesy.npz']
    z = np.load(str(iso2 / 'o_noeMap.npz'))
    assert 'H' not in z and 'H_blocks' not in z and 'frame' not in z and 'lags' not in z
    rows_a = [ln.split() for ln in open(str(sph / 'o_noesy.dat')) if not ln.startswith('#')]
    rows_b = [ln.split() for ln in open(str(iso2 / 'o_noesy.dat')) if not ln.startswith('#')]
    assert len(rows_a) == len(rows_b) == P + noe.n_pairs(P)
    for ra, rb in zip(rows_a, rows_b):
        assert ra[:4] == rb[:4] and all(last_digit_apart(x, y) for x, y in zip(ra[4:], rb[4:])), (ra, rb)
    zs = np.load(str(sph / 'o_noeMap.npz'))
    assert zs['H'].shape == (1, noe.n_pairs(P), 6) and 'lags' not in zs and zs['frame'].tolist() == [1.0, 0.0, 0.0, 0.0]
    rh = run_cli(tmp_path, 'rh', fn, lag_args + ['--noesyD', '1.1e7 1.6 0.4', '--vecRot', ' '.join('%.17g' % v for v in Q_F)])
    assert sorted(os.listdir(str(rh))) == ['o_noeMap.dat', 'o_noeMap.npz', 'o_noeMapCt.dat', 'o_noesy.dat', 'o_noesy.npz']
    zr = np.load(str(rh / 'o_noeMap.npz'))
    assert zr['lags'].tolist() == [0, 1, 2, 4, 8, 16] and zr['H'].shape == (6, noe.n_pairs(P), 6) and np.array_equal(zr['frame'], Q_F)
    res = noe.dipolar_map_superposed(xyz, ref32, fit, indexP, blocks=([0, 50, 100, 150], [50] * 4), mode=1, ctx=ctx, lags=[0, 1, 2, 4, 8, 16],
                                     dt=10.0, modes=True, frame=Q_F)
    assert zr['H'].tobytes() == res['H'].tobytes() and zr['H_blocks'].tobytes() == res['H_blocks'].tobytes()
    D = np.array(hm.ellipsoid_from_iso(1.1e7, 1.6, 0.4))
    want = noesy.noesy(dict(res, tau_e=res['tau_e'] * 1e-12, dt=res['dt'] * 1e-12), [0.05, 0.2], 600.0, D=D, tau_e='modes', ctx=ctx)
    zn = np.load(str(rh / 'o_noesy.npz'))
    for k in ('R', 'A'):
        assert zn[k].tobytes() == want[k].tobytes(), k
    assert not np.array_equal(zn['R'], np.load(str(iso2 / 'o_noesy.npz'))['R'])
