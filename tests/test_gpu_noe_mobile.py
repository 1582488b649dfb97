"""
GPU tests of the three tile kernels of csrc/sr_noe.hip (k_noe_pairs, k_noe_lagged, k_noe_modes: one workgroup body, csrc/sr_noe_tile.h)
and of spinrelax_amd.noe above them on MOBILE pairs: the star layout of tests/noe_inputs.py, whose 18 star pairs change their distance
by a factor up to 40 within a block (r^-6 over eight orders of magnitude, one frame holding up to all of a sum, C_dd passing through
zero, S2 from 0 to 0.87) beside 612 slow pairs 13 and more apart.  tests/test_noe_inputs_host.py asserts those conditions on the
same arrays and shows, with a float32 emulation of the kernels' operation sequence, that a correct kernel stays inside every bar here.

Every bar on a sum is the constant of the module that owns it, imported and unchanged (noe_inputs.ratios): they are relative to
sum r^-6, sum r^-3 or W per pair and so hold at any dynamic range.  The bars of this file are propagations of those, computed per pair:
  Cdd(k) = [sum_b G_b(k) / T] / A6, T = sum_b (n_b - k): with |dG| <= g W (g = BAR0 of the lagged map, 1e-12 in mode 1) and A6 within
    a relative (BAR0_A6, 1e-12): |dCdd| <= (g W / (T A6) + |Cdd| a) / (1 - a).  dCdd is std / (sqrt(B) - 1) of the per-block values:
    a standard deviation moves by at most the largest change of a value.
  tau_e is the integral of the positive part of the linear interpolant of Y(k) = (Cdd(k) - S2) / (1 - S2) up to its first zero:
    monotone in every Y(k), and Y is monotone in Cdd and in S2.  So tau_e lies between the values of the same host function at the
    lowest and at the highest Y over the four corners Cdd -+ its bar, S2 -+ its bar (BAR0_S2; 12e-12 in mode 1, test_gpu_noe.py),
    wherever 1 - S2 stays above the function's rigid threshold 1e-6 at every corner.  Below the threshold the documented value is 0:
    asserted in mode 1, where S2 is good to 1e-11; in mode 0 S2 of a rigid pair is 1 -+ 3e-5 and tau_e is only finite.
  mode_tau_e likewise with Y_m(k) = (g_m(k) - c_m) / (a_m - c_m): g = L H (L the matrix of noe.mode_amplitudes), |dg_m| <= sum_j |L_mj|
    bar_j W; c from the mean tensor T: |dT_ab| <= BAR0_T <r^-3>, |dQ| <= 6 |dT| (a rotation, the trace, a difference of two), the six
    products move by 2 |Q|max 6 |dT| + 36 |dT|^2 and c by L of that.
  The C(t) family (test_agrees_with_calculate_Ct_dipolar): see the test.
A share is the largest single term of a sum over the sum; "no frame dominates" means a share of at most 1/8, a classification, not a
tolerance.  Every test prints measured / bar per pair class (spike, contact, wide, other star, cross-star) before it asserts; the
device's figures are in docs/EXPERIMENTS.md section 39.
"""
import functools

import numpy as np
import pytest

import ct_dipolar_inputs as di
import noe_inputs as ni
from noe_inputs import BLOCKS, LAGS, LAGS_RAGGED, RAGGED, SPLIT_BLOCK, SPLIT_LAGS
from spinrelax_amd import ct as hostct
from spinrelax_amd import hip, noe
from test_gpu_ct_dipolar import oracle_core, planes_of
from test_gpu_noe import BAR0_A6, BAR0_S2, BAR0_T, rotmat
from test_gpu_noe_lagged import BAR0 as BAR0_G
from test_gpu_noe_modes import BAR0 as BAR0_H
from test_gpu_noe_modes import D_RHOMBIC, Q_F

pytestmark = pytest.mark.gpu

BAR1 = 1e-12
BAR1_S2 = 12 * BAR1                     # test_gpu_noe.py, test_rigid_body_without_quaternions
RIGID = 1e-6                            # noe.tau_e_from_Cdd: no internal term where 1 - S2 is below
DOMINATES = 0.125
TABLES = {'blocks': (BLOCKS, LAGS), 'ragged': (RAGGED, LAGS_RAGGED)}


@pytest.fixture(scope='module')
def ctx():
    c = hip.Context()
    assert c.noe_tile() == ni.TILE and c.noe_frame_batch() == ni.STAGE
    yield c
    c.close()


def split(blocks):
    return [b[0] for b in blocks], [b[1] for b in blocks]


def check(tag, got, ref, bl, mode, classes):
    worst = ni.report('\n' + tag, ni.ratios(got, ref, bl, mode), classes)
    assert all(np.isfinite(v).all() for k, v in got.items() if k != 'lags') and worst <= 1.0, tag


@functools.lru_cache(maxsize=None)
def device(c, name, table, mode, with_quat=True, with_frame=True):
    """the three kernels on one layout and block table, once per argument set: dict(sums, G, H, lags), read-only"""
    blocks, lags = TABLES[table] if table in TABLES else (SPLIT_BLOCK, SPLIT_LAGS)
    big, index, quat = ni.layout(name)
    bs, bl = split(blocks)
    q = quat if with_quat else None
    out = dict(sums=c.noe_pairs(big, index, quat=q, block_start=bs, block_len=bl, mode=mode),
               G=c.noe_lagged(big, index, list(lags), quat=q, block_start=bs, block_len=bl, mode=mode),
               H=c.noe_modes(big, index, list(lags), quat=q, frame=Q_F if with_frame else None, block_start=bs, block_len=bl, mode=mode),
               lags=tuple(lags))
    for k in ('sums', 'G', 'H'):
        out[k].setflags(write=False)
    return out


@pytest.mark.parametrize('mode', (0, 1))
@pytest.mark.parametrize('table', ('blocks', 'ragged'))
def test_pairs_against_the_oracle(ctx, table, mode):
    """the seven sums with the quaternions and without, and through noe.finalize reff6, reff3, S2rad, S2 and A3 of every block and of
    the total at the existing derived bars"""
    blocks, _ = TABLES[table]
    big, index, quat = ni.layout('A')
    bs, bl = split(blocks)
    assert ctx.noe_lagged_splits(36, max(bl), len(bl)) == ni.ksplit(36, max(bl), len(bl)) > 1
    for wq in (True, False):
        got = dict(sums=ctx.noe_pairs(big, index, quat=quat if wq else None, block_start=bs, block_len=bl, mode=mode))
        ref = ni.reference('A', blocks, (), wq, kinds=('sums',))
        check('map, %s, mode %d, %s' % (table, mode, 'quat' if wq else 'lab'), got, ref, bl, mode, ni.pair_classes(ni.ORDERS['A']))


@pytest.mark.parametrize('mode', (0, 1))
@pytest.mark.parametrize('table', ('blocks', 'ragged'))
def test_lagged_against_the_oracle(ctx, table, mode):
    """G at the lags 0, 1, 3, 16, 17, 129, 499 and 999 (one term) of the blocks of 1000 frames, at lag 0 of the ragged table (its
    shortest block has one frame), with the quaternions and without; G(0) against the map's own r^-6 sums at BAR_LAG0"""
    blocks, lags = TABLES[table]
    big, index, quat = ni.layout('A')
    bs, bl = split(blocks)
    for wq in (True, False):
        q = quat if wq else None
        got = dict(G=ctx.noe_lagged(big, index, list(lags), quat=q, block_start=bs, block_len=bl, mode=mode), lags=lags,
                   sums=ctx.noe_pairs(big, index, quat=q, block_start=bs, block_len=bl, mode=mode))
        ref = ni.reference('A', blocks, lags, wq, kinds=('sums', 'G'))
        check('lagged, %s, mode %d, %s' % (table, mode, 'quat' if wq else 'lab'), got, ref, bl, mode, ni.pair_classes(ni.ORDERS['A']))


@pytest.mark.parametrize('mode', (0, 1))
@pytest.mark.parametrize('table', ('blocks', 'ragged'))
def test_modes_against_the_oracle(ctx, table, mode):
    """the six mode sums with (quat, Q_F), (None, Q_F) and (quat, None), each component against its own bar, and the identity
    2.25 H0 + 0.75 H1 + 3 (H3 + H4 + H5) = G at BAR_IDENT"""
    blocks, lags = TABLES[table]
    big, index, quat = ni.layout('A')
    bs, bl = split(blocks)
    for wq, wf in ((True, True), (False, True), (True, False)):
        q = quat if wq else None
        got = dict(H=ctx.noe_modes(big, index, list(lags), quat=q, frame=Q_F if wf else None, block_start=bs, block_len=bl, mode=mode),
                   G=ctx.noe_lagged(big, index, list(lags), quat=q, block_start=bs, block_len=bl, mode=mode))
        ref = ni.reference('A', blocks, lags, wq, wf, kinds=('G', 'H'))
        check('modes, %s, mode %d, %s, %s' % (table, mode, 'quat' if wq else 'lab', 'frame' if wf else 'no frame'), got, ref, bl, mode,
              ni.pair_classes(ni.ORDERS['A']))


@pytest.mark.parametrize('mode', (0, 1))
def test_frame_splits(ctx, mode):
    """one draw (18 atoms, one tile) and one block of 3016 frames: 23 frame splits (asserted: at least 2), partial tiles added by
    k_noe_finish.  At lag 129 the spike frame 1222 is an origin of split 9 and the frame t + k of an origin of split 8 (asserted from
    noe_lag_origins' rule, restated in noe_inputs.lag_origins); lag 1500 leaves splits of 66 origins.  All three kernels."""
    S = ctx.noe_lagged_splits(18, ni.N_FRAMES, 1)
    assert S == ni.ksplit(18, ni.N_FRAMES, 1) >= 2
    sf, k = di.spike_frame(ni.N_FRAMES, ni.SEEDS[0]), 129
    owner = [[s for s in range(S) if ni.lag_origins(ni.N_FRAMES, k, S, s)[0] <= t < ni.lag_origins(ni.N_FRAMES, k, S, s)[1]] for t in (sf, sf - k)]
    assert k in SPLIT_LAGS and len(owner[0]) == len(owner[1]) == 1 and owner[0] != owner[1]
    got = device(ctx, 'one', 'split', mode)
    ref = ni.reference('one', SPLIT_BLOCK, SPLIT_LAGS)
    check('frame splits, mode %d' % mode, got, ref, [ni.N_FRAMES], mode, ni.pair_classes(ni.ORDERS['one']))


# ---- the derived functions where they are at their edges ---------------------------------------------------------------------------
def cdd_bars(ref, fin, bl, lags, mode):
    """(bar of Cdd (K, npairs), bar of dCdd) by the propagation of the module docstring"""
    g, a = (BAR1, BAR1) if mode else (BAR0_G, BAR0_A6)
    bl, lg = np.asarray(bl), np.asarray(lags)
    terms = (bl[:, None] - lg[None, :]).astype(np.float64)                     # (B, K)
    C = ref['G'].sum(axis=0) / terms.sum(axis=0)[:, None] / fin['A6'][None]
    bar = (g * ref['W'].sum(axis=0) / terms.sum(axis=0)[:, None] / fin['A6'][None] + np.abs(C) * a) / (1 - a)
    C_b = ref['G'] / terms[:, :, None] / fin['A6_b'][:, None, :]
    bar_b = (g * ref['W'] / terms[:, :, None] / fin['A6_b'][:, None, :] + np.abs(C_b) * a) / (1 - a)
    return bar, (bar_b.max(axis=0) / (np.sqrt(bl.size) - 1.0) if bl.size > 1 else bar_b.max(axis=0))


def tau_bounds(n_lo, n_hi, d_lo, d_hi, lags, dt=1.0):
    """tau_e between the host function's values at the lowest and the highest Y = n / d over the corners; d_lo > 0"""
    Y_lo = np.where(n_lo >= 0, n_lo / d_hi, n_lo / d_lo)
    Y_hi = np.where(n_hi >= 0, n_hi / d_lo, n_hi / d_hi)
    zero = np.zeros(Y_lo.shape[1])
    return noe.tau_e_from_Cdd(Y_lo, zero, lags, dt), noe.tau_e_from_Cdd(Y_hi, zero, lags, dt)


@pytest.mark.parametrize('with_quat', (True, False), ids=('quat', 'lab'))
@pytest.mark.parametrize('mode', (0, 1))
def test_derived_functions_at_their_edges(ctx, mode, with_quat):
    """noe.dipolar_map(..., lags, modes=True, frame=Q_F) on the three blocks: Cdd and dCdd against the oracle's at the propagated bar
    (Cdd passes through zero on the star pairs); tau_e and mode_tau_e finite and between the values of the same host functions on the
    oracle's sums at the corners of the bars (module docstring); tau_e = 0 where the oracle's 1 - S2 is below 1e-6 (the pairs of two
    centres, in the lab frame; mode 1); nothing non-finite anywhere, the const and the spike pairs included"""
    big, index, quat = ni.layout('A')
    bs, bl = split(BLOCKS)
    lags = list(LAGS)
    cls = ni.pair_classes(ni.ORDERS['A'])
    res = noe.dipolar_map(big, index, quat=quat if with_quat else None, blocks=(bs, bl), mode=mode, ctx=ctx, lags=lags, modes=True, frame=Q_F)
    for k in ('sums', 'G', 'H', 'Cdd', 'dCdd', 'tau_e', 'dtau_e', 'S2', 'S2rad', 'reff6', 'reff3', 'Cdd_b', 'tau_e_b'):
        assert np.isfinite(res[k]).all(), k
    mte = noe.mode_tau_e(res, D_RHOMBIC)
    assert np.isfinite(mte).all() and mte.min() >= 0 and res['tau_e'].min() >= 0
    ref = ni.reference('A', BLOCKS, LAGS, with_quat, True)
    fin = noe.finalize(ref['sums'], bl)
    want = noe.finalize_lagged(ref['G'], bl, lags, fin)
    tag = '\nderived, mode %d, %s' % (mode, 'quat' if with_quat else 'lab')
    # Cdd, dCdd
    bar, dbar = cdd_bars(ref, fin, bl, lags, mode)
    rat = dict(Cdd=np.max(np.abs(res['Cdd'] - want['Cdd']) / bar, axis=0), dCdd=np.max(np.abs(res['dCdd'] - want['dCdd']) / dbar, axis=0))
    sp = ni.star_pairs(ni.ORDERS['A'])
    assert np.any((want['Cdd'][:, sp].min(axis=0) < 0) & (want['Cdd'][:, sp].max(axis=0) > 0.9))         # a sign change inside the lag list
    worst = ni.report(tag, rat, cls)
    assert worst <= 1.0
    # tau_e
    bS2 = BAR1_S2 if mode else BAR0_S2
    one = 1.0 - fin['S2']
    flex, rigid = one - bS2 >= RIGID, one < RIGID
    n_lo, n_hi = want['Cdd'] - bar - (fin['S2'] + bS2)[None], want['Cdd'] + bar - (fin['S2'] - bS2)[None]
    lo, hi = tau_bounds(n_lo, n_hi, np.where(flex, one - bS2, 1.0)[None], (one + bS2)[None], lags)
    got = res['tau_e']
    inside = (got >= lo * (1 - 1e-12)) & (got <= hi * (1 + 1e-12))
    width = np.where(flex, hi - lo, 0.0)
    print('tau_e: %d pairs between the corner values (widest interval %.3g frames, at tau_e %.3g; of the star pairs %.3g), %d rigid, %d next to '
          'the threshold' % (flex.sum(), width.max(), want['tau_e'][np.argmax(width)], width[sp].max(), rigid.sum(), (~flex & ~rigid).sum()))
    assert flex[sp].all() and np.all(inside[flex]), np.nonzero(flex & ~inside)[0]
    assert want['tau_e'][sp].max() > 1.0                                                          # there is something to integrate
    if not with_quat:
        assert rigid.sum() >= 18 * 17 // 2                                                        # every pair of two centres
    if mode == 1:
        assert np.all(got[rigid] == 0.0)
    # mode_tau_e
    wm = noe.finalize_modes(ref['H'], bl, lags, Q_F)
    T = (np.asarray(bl)[:, None] - np.asarray(lags)[None, :]).sum(axis=0).astype(np.float64)
    g, c = noe.mode_amplitudes(wm['H'], D_RHOMBIC), np.clip(noe.mode_plateau(fin['T'], D_RHOMBIC, Q_F), 0.0, None)      # (K, n, 5), (n, 5)
    L = np.abs(np.stack([noe.mode_amplitudes(e, D_RHOMBIC) for e in np.eye(6)], axis=1))                                 # (5, 6)
    bH = np.full(6, BAR1) if mode else BAR0_H
    dg = (ref['W'].sum(axis=0) / T[:, None])[..., None] * (L @ bH)[None, None, :]
    dT = (BAR1 if mode else BAR0_T) * fin['A3']
    Fm = rotmat(Q_F[None])[0]
    Q = np.einsum('ab,nbc,dc->nad', Fm, fin['T'], Fm)
    Qmax = 2 * np.maximum(np.abs(Q).max(axis=(1, 2)), fin['A3'])          # |qz| <= |Q_zz| + tr / 3, |dl| <= 2 max |Q_ab|
    dc = (2 * Qmax * 6 * dT + 36 * dT * dT)[:, None] * L.sum(axis=1)[None, :]
    a, da = g[0], dg[0]
    robust = (a - da > 0) & ((a - c) - (da + dc) > RIGID * (a + da))
    n_lo, n_hi = (g - c[None] - dg - dc[None]), (g - c[None] + dg + dc[None])
    d_lo, d_hi = np.where(robust, (a - c) - (da + dc), 1.0), (a - c) + (da + dc)
    K = len(lags)
    lo, hi = tau_bounds(n_lo.reshape(K, -1), n_hi.reshape(K, -1), d_lo.reshape(1, -1), d_hi.reshape(1, -1), lags)
    lo, hi = lo.reshape(a.shape), hi.reshape(a.shape)
    inside = (mte >= lo * (1 - 1e-12)) & (mte <= hi * (1 + 1e-12))
    print('mode_tau_e: %d of %d (pair, mode) between the corner values, widest interval %.3g frames' % (robust.sum(), robust.size, np.where(robust, hi - lo, 0).max()))
    assert robust[sp].any() and np.all(inside[robust]), np.argwhere(robust & ~inside)[:5]
    want_m = noe.mode_tau_e(dict(wm, T=fin['T'], lags=np.asarray(lags), dt=1.0), D_RHOMBIC)
    assert np.all((want_m >= lo * (1 - 1e-12))[robust]) and np.all((want_m <= hi * (1 + 1e-12))[robust])     # the bounds hold the oracle's own


# ---- reproducibility -------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes_and_a_lag_alone_its_bits(ctx):
    big, index, quat = ni.layout('A')
    bs, bl = split(BLOCKS)
    lags = list(LAGS)
    for mode in (0, 1):
        kw = dict(quat=quat, block_start=bs, block_len=bl, mode=mode)
        first = device(ctx, 'A', 'blocks', mode)
        assert ctx.noe_pairs(big, index, **kw).tobytes() == first['sums'].tobytes()
        assert ctx.noe_lagged(big, index, lags, **kw).tobytes() == first['G'].tobytes()
        assert ctx.noe_modes(big, index, lags, frame=Q_F, **kw).tobytes() == first['H'].tobytes()
        for q in (0, 5, 7):                                           # lag 0, 129 and the single-term 999
            assert ctx.noe_lagged(big, index, [lags[q]], **kw)[:, 0].tobytes() == first['G'][:, q].tobytes(), (mode, lags[q])
            assert ctx.noe_modes(big, index, [lags[q]], frame=Q_F, **kw)[:, 0].tobytes() == first['H'][:, q].tobytes(), (mode, lags[q])


@pytest.mark.parametrize('mode', (0, 1))
@pytest.mark.parametrize('name', ('B', 'C'))
def test_other_tiles_same_oracle(ctx, name, mode):
    """the layouts B and C move star pairs into other tiles (with A every class of pair is computed in every tile pair): all three
    kernels within the bars of the same oracle; the sums need not be bit-equal to those of A"""
    got = device(ctx, name, 'blocks', mode)
    ref = ni.reference(name, BLOCKS, LAGS)
    check('layout %s, mode %d' % (name, mode), got, ref, split(BLOCKS)[1], mode, ni.pair_classes(ni.ORDERS[name]))


# ---- systematic error ------------------------------------------------------------------------------------------------------------
def test_no_systematic_error_where_no_frame_dominates(ctx):
    """tests/test_gpu_noe.py: an error above a quarter of a bar over many frames points at a systematic error.  Asserted on every sum
    (block, lag, pair) of mode 0 in which no single term holds more than 1/8: r^-6 and the tensor sums of the map, G, H0 .. H5."""
    got = device(ctx, 'A', 'blocks', 0)
    ref = ni.reference('A', BLOCKS, LAGS)
    pm = ni.pair_map(ni.ORDERS['A'])
    s6, s3, sW = (v[..., pm] for v in ni.shares(2, BLOCKS, LAGS))
    cls = ni.pair_classes(ni.ORDERS['A'])
    err = {'A6': np.where(s6 <= DOMINATES, np.abs(got['sums'][..., 0] / ref['sums'][..., 0] - 1) / BAR0_A6, 0.0),
           'T': np.where(s3 <= DOMINATES, np.max(np.abs(got['sums'][..., 1:] - ref['sums'][..., 1:]), axis=-1) / ref['r3'] / BAR0_T, 0.0),
           'G': np.where(sW <= DOMINATES, np.abs(got['G'] - ref['G']) / ref['W'] / BAR0_G, 0.0)}
    for m in range(6):
        err['H%d' % m] = np.where(sW <= DOMINATES, np.abs(got['H'][..., m] - ref['H'][..., m]) / ref['W'] / BAR0_H[m], 0.0)
    assert (s6 <= DOMINATES).mean() > 0.99 and (sW[:, :-1] <= DOMINATES).mean() > 0.99 and not (sW[:, -1] <= DOMINATES).any()
    assert (s6[:, ni.star_pairs(ni.ORDERS['A'])] > 0.8).sum() == 2                          # the two spikes are not in it
    worst = ni.report('\nno frame dominates, mode 0', {k: v.reshape(-1, v.shape[-1]).max(axis=0) for k, v in err.items()}, cls)
    assert worst <= 0.25


# ---- the C(t) family --------------------------------------------------------------------------------------------------------------
def test_agrees_with_calculate_Ct_dipolar(ctx):
    """test_gpu_noe_lagged.py's test on a WIDE, a CONTACT and the SPIKE star pair, block 1 (which holds the spike) as the chunk, both
    sides in mode 1.  The bar is each side's own bar against the float64 definition on the exact d', added.
    The map: cdd_bars in mode 1.
    calculate_Ct_dipolar gets float32(d') and packs float32 planes a = d' sqrt(w) / r and w = (r_ref / r)^3: the pack's 1e-7 on a and w
    (tests/test_gpu_ct_dipolar.py), and the rounding of the vectors handed over, 2^-24 relative per component: r and r_ref move by
    2^-24, w by 6 2^-24 w, a component of a by (1 + 1 + 1.5) 2^-24 |a|, |a| = sqrt(w).  So e_a(t) = 1e-7 + 3.5 2^-24 sqrt(w) per
    component and e_w(t) = 1e-7 + 6 2^-24 w, propagated through the definition C = [1.5 sum (a . a')^2 - 0.5 sum w w'] / (F - k) / n,
    n = sum w^2 / F, on the oracle's planes:
    |d (a . a')| <= sqrt(3) (|a| e_a' + |a'| e_a), |d (a . a')^2| <= 2 |a||a'| that, |d (w w')| <= w e_w' + w' e_w, |dn| <= sum 2 w e_w / F;
    the mode-1 kernel adds its 1e-12."""
    F = 1000
    big, index, quat = ni.layout('A')
    fr = slice(1000, 2000)
    lags = [k for k in LAGS if 1 <= k <= F // 2]
    stars = [ni.star(0, di.FAST_WIDE), ni.star(0, di.JUMP_CONTACT), ni.star(0, di.FAST_SPIKE)]
    pick = ni.star_pairs(ni.ORDERS['A'])[stars]
    res = noe.dipolar_map(big[fr], index, quat=quat[fr], mode=1, ctx=ctx, lags=lags)
    pr = res['pairs'][pick]
    x = big[fr][:, index].astype(np.float64)
    d = np.einsum('tab,tpb->tpa', rotmat(quat[fr]), x[:, pr[:, 1]] - x[:, pr[:, 0]])
    Ct = hostct.calculate_Ct_dipolar(d.astype(np.float32)[None], ctx=ctx, mode=1)[0]
    got_ct = Ct[np.array(lags) - 1]
    # the definition on the exact d', and both bars
    a, w, _ = planes_of(d)
    want = oracle_core(a[None], w[None], lags)[0]
    ref = {k: v[:, :, ni.pair_map(ni.ORDERS['A'])[pick]] for k, v in zip(('G', 'W'), ni.ref_G(2, True, ((1000, 1000),), tuple(lags)))}
    s, _ = ni.ref_sums(2, True, ((1000, 1000),))
    fin = noe.finalize(s[:, ni.pair_map(ni.ORDERS['A'])[pick]], [F])
    bar_map, _ = cdd_bars(ref, fin, [F], lags, 1)
    assert np.max(np.abs(ref['G'][0] / (F - np.array(lags))[:, None] / fin['A6'][None] - want)) < 1e-12      # one definition, two spellings
    ea, ew = 1e-7 + 3.5 * 2.0 ** -24 * np.sqrt(w), 1e-7 + 6 * 2.0 ** -24 * w
    n = (w * w).sum(axis=0) / F
    dn = (2 * w * ew).sum(axis=0) / F
    bar_ct = np.empty_like(want)
    for m, k in enumerate(lags):
        w0, w1, a0, a1 = w[:F - k], w[k:], np.sqrt(w[:F - k]), np.sqrt(w[k:])
        dnum = (1.5 * 2 * a0 * a1 * np.sqrt(3.0) * (a0 * ea[k:] + a1 * ea[:F - k]) + 0.5 * (w0 * ew[k:] + w1 * ew[:F - k])).sum(axis=0) / (F - k)
        bar_ct[m] = (dnum / n + np.abs(want[m]) * dn / n) / (1 - dn / n) + BAR1
    e_map, e_ct, e = np.abs(res['Cdd'][:, pick] - want), np.abs(got_ct - want), np.abs(res['Cdd'][:, pick] - got_ct)
    print('\nCdd of a wide, a contact and the spike pair, map against calculate_Ct_dipolar: %s (bars %s); the map against the definition '
          '%.3g of its bar, calculate_Ct_dipolar %.3g of its' % (np.max(e, axis=0), np.max(bar_map + bar_ct, axis=0), np.max(e_map / bar_map),
                                                               np.max(e_ct / bar_ct)))
    assert np.all(e_map <= bar_map) and np.all(e_ct <= bar_ct) and np.all(e <= bar_map + bar_ct)
