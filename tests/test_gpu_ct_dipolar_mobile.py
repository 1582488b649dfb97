"""
GPU tests (marker gpu) of the distance-weighted correlation functions on MOBILE pairs whose distance varies by factors: the direct
forms (k_dipolar_rmin, k_pack_dipolar, k_ct_dipolar, k_ct_dipolar_cross, their _norm kernels and k_ct_cross_p0) and the blocked forms
(csrc/sr_ct_dipolar_long.hip) on the nine series of ct_dipolar_inputs.mixed -- wobble x mild beside tumbling, jumping and uncorrelated
directions under log-normal (sigma 0.5), two-state contact, orientation-tied, one-frame-spike and constant distances -- against the
definition in float64 (the lag-by-lag oracles of tests/test_gpu_ct_dipolar*.py up to 4100 frames, their FFT forms beyond).  The
conditions that make the inputs hard are asserted without a GPU in tests/test_ct_dipolar_inputs_host.py.

Bars, all ABSOLUTE at scale = max(1, max_t |C_ref|) per series or pair (ct_inputs.close; C_dd of these series passes through zero):
  * the pack: 1e-7 absolute on a and w, w == 1 at the frame of r_ref, the other frames of the spike series below 1e-3;
  * mode 1 (float64) against the definition on the planes the pack wrote: 1e-12 on C, dC, P0, dP0; 1e-12 relative on <w>, <w^2>;
  * mode 0, direct forms: 1e-6 (the north star) on C, dC, P0 and dP0; reff6, reff3 and S2rad 1e-6 relative;
  * mode 0, blocked forms: 1e-6 AND, per series, 4 x the error of ct_dipolar_inputs.emulate_dipolar_f32 (scipy's float32 transforms,
    means restored in float64) on the same chunks; a pair takes the larger of its two series' bars.
Every test prints its measured error per series next to the bar; docs/EXPERIMENTS.md section 38 is filled from those prints.

Measured on MI355X, worst over the lengths of this module, in the order of ct_dipolar_inputs.SERIES (wobble*mild, walk.02*wide,
walk.15*wide, jump*contact, white*contact, walk.02*angle, walk.15*spike, walk.02*const, shared*contact):
  direct, mode 0   |dC| / scale           4.4e-8 1.4e-7 1.1e-7 9.4e-8 8.4e-8 5.2e-8 8.6e-8 3.4e-8 8.4e-8
                   |d dC| (sqrt(R) - 1)   4.0e-8 1.9e-7 1.5e-7 1.3e-7 1.1e-7 7.8e-8 1.2e-7 3.4e-8 1.2e-7
  blocked, mode 0  |dC| / scale           3.9e-8 9.0e-8 1.1e-7 1.5e-7 1.9e-8 7.6e-8 4.1e-8 8.4e-8 1.1e-7
                   |d dC| (sqrt(R) - 1)   9.3e-9 1.1e-7 6.4e-8 1.8e-7 2.6e-8 9.3e-8 5.8e-8 2.3e-8 1.5e-7
                   kernel / emulation     1.3    1.4    1.7    2.3    1.2    0.94   0.95   0.81   1.6      (bar 2: 4)
  pairs (wide(i,i), contact(i,i), slow-fast, fast-slow, independent, shared), mode 0:
    direct   |dC| 1.1e-7 9.4e-8 6.7e-8 7.3e-8 8.0e-8 5.9e-8   |dP0| 3.7e-8 8.7e-8 1.7e-8 1.7e-8 1.2e-8 5.1e-9   |d dC| <= 1.3e-7, |d dP0| <= 1.2e-7
    blocked  |dC| 1.2e-7 1.6e-7 9.6e-9 8.8e-9 2.5e-8 1.8e-8   |dP0| 6.2e-9 4.0e-8 2.1e-10 2.1e-10 1.1e-10 1.4e-9  |d dC| <= 2.1e-7, |d dP0| <= 5.4e-8
  mode 1: direct forms <= 1.1e-15, blocked forms <= 3.6e-14 (k_dipl_f64 sums one lag per thread, frames in order).
Every series meets both bars.  Two checks of this module failed on the kernels as they were, and the kernels were changed:
  * mode 1 on the spike series: 1.2e-12 (F = 4100) .. 3.6e-12 (12 289), and 7.7e-14 .. 2.0e-13 on jump*contact.  The raw sums carried
    (F - k) / 3 so that kernel 1's finalizer (1.5 S / n - 0.5) could be reused; that rounds the unnormalised function to 1e-16 absolute,
    and the division by <w^2> (3e-5 for one close frame in 36 000) makes 4e-12 of it.  The sums now leave without the constant and the
    finalizer subtracts nothing for them: 4.9e-19 and 5.6e-16.
  * (i, j) and (j, i) with sym = 1 in the direct pair kernel differed in the last bit at single lags (F = 1000, lag 478): the two
    directions were added into one sum in the order the pair names them.  A symmetric pair now runs with its lower vector first.
"""
import contextlib

import numpy as np
import pytest

import ct_dipolar_inputs as di
import ct_inputs as ci
from conftest import relerr
from ct_dipolar_inputs import PAIRS, R, SERIES
from spinrelax_amd import ct as hostct
from test_ct_dipolar_long_host import fft_core, fft_cross_core
from test_gpu_ct_dipolar import dev_ct as dev_ct_auto
from test_gpu_ct_dipolar import dev_pack, oracle_core as core_auto, planes_of
from test_gpu_ct_dipolar_cross import dev_ct as dev_ct_pair
from test_gpu_ct_dipolar_cross import oracle_core as core_pair

pytestmark = pytest.mark.gpu

V = di.NSER
RTOL = 1e-6
AUTO_DIRECT = [128, 257, 1000, 4100]       # the float64 path alone; one-wave slabs; lags behind the last full block; four-wave workgroup
PAIR_DIRECT = [257, 1000, 4100]
# (F, value of "ct_dipolar_long_min_frames"): 5462 by the lowered option, the others through the default dispatch
AUTO_BLOCKED = [(5462, 5462), (10017, 10017), (12289, 10017)]
PAIR_BLOCKED = [(4097, 4097), (4897, 4897), (8193, 4897)]
DEFAULTS = dict(ct_dipolar_long_min_frames=10017, ct_dipolar_cross_long_min_frames=4897)


@pytest.fixture(scope='module')
def ctx():
    from spinrelax_amd.hip import Context
    c = Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def options(ctx, **kw):
    """both options are set, to kw's value or to the default, and the defaults are back afterwards"""
    assert set(kw) <= set(DEFAULTS)
    try:
        for k, val in {**DEFAULTS, **kw}.items():
            ctx.set_option(k, val)
        yield
    finally:
        for k, val in DEFAULTS.items():
            ctx.set_option(k, val)


def fmt(names, e):
    return ' '.join('%s %.1e' % kv for kv in zip(names, e))


def report(tag, F, names, C, dC, Cr, dCr, bar2=None, emu=None):
    eC, eD = ci.errors(C, dC, Cr, dCr, R)
    print('\n[dipolar mobile] %s F=%d  |dC|/scale   %s' % (tag, F, fmt(names, eC)))
    print('[dipolar mobile] %s F=%d  |d dC|(sqrt(R)-1)/scale   %s' % (tag, F, fmt(names, eD)))
    if emu is not None:
        print('[dipolar mobile] %s F=%d  emulation |dC|/scale   %s' % (tag, F, fmt(names, emu)))
        print('[dipolar mobile] %s F=%d  bar 2   %s' % (tag, F, fmt(names, bar2)))
        with np.errstate(divide='ignore'):
            print('[dipolar mobile] %s F=%d  kernel / emulation   %s' % (tag, F, fmt(names, eC / emu)))
    return eC, eD


def same_bytes(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def all_finite(got):
    return all(np.all(np.isfinite(g)) for g in got)


def raw4(F):
    return di.case_input(F)[2][:R * F].reshape(R, F, V, 3)


def planes_from(p, F, starts=None):
    """a4 (R, F, V, 3), w4 (R, F, V) float64 of the downloaded planes p (V, 4, Npad)"""
    st = np.arange(R) * F if starts is None else starts
    a = p[:, :3].transpose(2, 0, 1).astype(np.float64)                    # (Npad, V, 3)
    w = p[:, 3].T.astype(np.float64)
    return np.stack([a[s:s + F] for s in st]), np.stack([w[s:s + F] for s in st])


# ---- the pack ----------------------------------------------------------------------------------------------------------------------------
def test_pack_on_the_mixed_input(ctx):
    """both input forms, a frame count that is no multiple of the tile: w spans 1 .. 1e-4 in one launch"""
    F = 257
    u, d, raw = di.case_input(F)
    N = raw.shape[0]
    assert N % 64 != 0
    for form, vec, dist in (('raw', raw, None), ('dist', u, d)):
        p, rref, _, Npad = dev_pack(ctx, vec, dist)
        a, w, rr = planes_of(vec, dist)
        r = np.sqrt((vec.astype(np.float64) ** 2).sum(-1)) if dist is None else dist.astype(np.float64)
        ea, ew = np.max(np.abs(p[:, :3, :N] - a.transpose(1, 2, 0)), axis=(1, 2)), np.max(np.abs(p[:, 3, :N] - w.T), axis=1)
        print('\n[dipolar mobile] pack %s  |da|   %s' % (form, fmt(SERIES, ea)))
        print('[dipolar mobile] pack %s  |dw|   %s   r_ref %.1e   min w %.1e' % (form, fmt(SERIES, ew), relerr(rref, rr), p[:, 3, :N].min()))
        assert np.max(ea) <= 1e-7 and np.max(ew) <= 1e-7
        assert relerr(rref, rr) <= 1e-14
        assert np.all(p[:, :, N:] == 0.0)
        at = np.argmin(r, axis=0)
        assert np.all(p[np.arange(V), 3, at] == 1.0) and np.max(p[:, 3]) == 1.0          # the frame of r_ref itself has w = 1
        spike = p[di.FAST_SPIKE, 3, :N]
        assert np.count_nonzero(spike == 1.0) == 1 and np.max(np.delete(spike, at[di.FAST_SPIKE])) < 1e-3
        assert p[:, 3, :N].min() < 1e-3 and np.all(p[:, 3, :N] > 0.0)


# ---- the direct autocorrelation form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', AUTO_DIRECT)
def test_direct_autocorrelation_float64(ctx, F):
    """mode 1 against the definition on the planes the pack wrote"""
    raw = di.case_input(F)[2][:R * F]
    p, rref, planes, Npad = dev_pack(ctx, raw, None)
    C, dC, wm = dev_ct_auto(ctx, planes, Npad, V, R, F, 1)
    a4, w4 = planes_from(p, F)
    Cr, dCr, w1, w2 = core_auto(a4, w4)
    report('direct auto mode 1', F, SERIES, C, dC, Cr, dCr)
    assert ci.close(C, dC, Cr, dCr, R, ci.BAR_F64)
    assert relerr(wm[:, 0], w1) <= 1e-12 and relerr(wm[:, 1], w2) <= 1e-12
    assert relerr(rref, planes_of(raw, None)[2]) <= 1e-14


def check_auto(tag, F, got, ref, bar, b2=None, emu=None):
    report(tag, F, SERIES, got[0], got[1], ref[0], ref[1], b2, emu)
    print('[dipolar mobile] %s F=%d  reff6 %.1e reff3 %.1e S2rad %.1e' % ((tag, F) + tuple(relerr(g, w) for g, w in zip(got[2:], ref[2:]))))
    assert got[0].shape == got[1].shape == (F // 2, V)
    assert all_finite(got)                                             # the spike series and the chunks without a contact too
    assert ci.close(got[0], got[1], ref[0], ref[1], R, bar), (tag, F)
    if b2 is not None:
        assert ci.close(got[0], got[1], ref[0], ref[1], R, b2), (tag, F, 'bar 2', b2)
    for g, w in zip(got[2:], ref[2:]):
        assert relerr(g, w) < RTOL


def check_const_series(ctx, tag, F, got):
    """the series at a constant distance is kernel 1's C(t) of the same unit vectors: two results within the bar of one definition"""
    u = di.case_input(F)[0][:R * F].reshape(R, F, V, 3)
    Cp, dCp = hostct.calculate_Ct_Palmer(u[:, :, di.SLOW_CONST:di.SLOW_CONST + 1], ctx=ctx, mode=0)
    k = di.SLOW_CONST
    eC, eD = ci.errors(got[0][:, k:k + 1], got[1][:, k:k + 1], Cp, dCp, R)
    print('[dipolar mobile] %s F=%d  constant distance against calculate_Ct_Palmer   |dC| %.1e |d dC| %.1e' % (tag, F, eC[0], eD[0]))
    assert ci.close(got[0][:, k:k + 1], got[1][:, k:k + 1], Cp, dCp, R, ci.NORTH_STAR)


@pytest.mark.parametrize('F', AUTO_DIRECT)
def test_direct_autocorrelation_float32(ctx, F):
    ref = di.reference_auto(F)
    assert F <= ctx.ct_dipolar_max_frames() and F < ctx.ct_dipolar_long_min_frames
    with options(ctx):
        got = hostct.calculate_Ct_dipolar(raw4(F), ctx=ctx, mode=0)
        check_auto('direct auto mode 0', F, got, ref, ci.NORTH_STAR)
        assert same_bytes(got, hostct.calculate_Ct_dipolar(raw4(F), ctx=ctx, mode=0))          # two runs: the same bytes
        check_const_series(ctx, 'direct auto', F, got)
        if F == 257:
            # the other input form: unit vectors and the distances beside them
            u, d, _ = di.case_input(F)
            alt = hostct.calculate_Ct_dipolar(u[:R * F].reshape(R, F, V, 3), dist=d[:R * F].reshape(R, F, V), ctx=ctx, mode=0)
            check_auto('direct auto mode 0, dist given', F, alt, di.reference_auto(F, 'dist'), ci.NORTH_STAR)
            check_const_series(ctx, 'direct auto, dist given', F, alt)


# ---- the direct pair form --------------------------------------------------------------------------------------------------------------------
def check_pairs(tag, F, got, ref, bar, b2=None):
    P0, dP0, C, dC, reff6 = got
    P0r, dP0r, Cr, dCr, reff6r = ref
    report(tag, F, di.PAIR_NAMES, C, dC, Cr, dCr)
    eP, edP = di.errors_p0(P0, dP0, P0r, dP0r)
    print('[dipolar mobile] %s F=%d  |dP0|/scale   %s' % (tag, F, fmt(di.PAIR_NAMES, eP)))
    print('[dipolar mobile] %s F=%d  |d dP0|(sqrt(R)-1)/scale   %s   reff6 %.1e   P0 %s' % (tag, F, fmt(di.PAIR_NAMES, edP), relerr(reff6, reff6r),
                                                                                            np.round(P0r, 4)))
    assert C.shape == dC.shape == (F // 2, len(PAIRS)) and reff6.shape == (len(PAIRS), 2)
    assert all_finite(got)
    assert ci.close(C, dC, Cr, dCr, R, bar) and di.close_p0(P0, dP0, P0r, dP0r, bar), (tag, F)
    if b2 is not None:
        print('[dipolar mobile] %s F=%d  bar 2 per pair   %s' % (tag, F, fmt(di.PAIR_NAMES, b2)))
        assert ci.close(C, dC, Cr, dCr, R, b2), (tag, F, 'bar 2', b2)
    assert relerr(reff6, reff6r) < RTOL


def check_pair_identities(tag, F, sym, got, ref, auto, bar):
    """(i, i) is the autocorrelation form with P0 = 1; a repeated pair: the same bytes; (i, j) and (j, i): the same bytes for sym = 1 and
    another function for sym = 0"""
    P0, dP0, C, dC, reff6 = got
    for p in (di.P_II_WIDE, di.P_II_CONTACT):
        v = PAIRS[p, 0]
        eC, eD = ci.errors(C[:, p:p + 1], dC[:, p:p + 1], auto[0][:, v:v + 1], auto[1][:, v:v + 1], R)
        print('[dipolar mobile] %s F=%d sym=%d  pair (%d, %d) against the autocorrelation form   |dC| %.1e |d dC| %.1e   P0 - 1 = %.1e'
              % (tag, F, sym, v, v, eC[0], eD[0], P0[p] - 1.0))
        assert ci.close(C[:, p:p + 1], dC[:, p:p + 1], auto[0][:, v:v + 1], auto[1][:, v:v + 1], R, bar)
        assert abs(P0[p] - 1.0) <= bar
    a, b = di.P_IJ, di.P_REPEAT
    assert C[:, a].tobytes() == C[:, b].tobytes() and dC[:, a].tobytes() == dC[:, b].tobytes()
    assert P0[a].tobytes() == P0[b].tobytes() and dP0[a].tobytes() == dP0[b].tobytes() and reff6[a].tobytes() == reff6[b].tobytes()
    if sym:
        assert C[:, di.P_IJ].tobytes() == C[:, di.P_JI].tobytes() and P0[di.P_IJ].tobytes() == P0[di.P_JI].tobytes()
    else:
        assert np.max(np.abs(ref[2][:, di.P_IJ] - ref[2][:, di.P_JI])) > 1e-4
        assert np.max(np.abs(C[:, di.P_IJ] - C[:, di.P_JI])) > 1e-4


@pytest.mark.parametrize('F', PAIR_DIRECT)
def test_direct_pairs_float64(ctx, F):
    """mode 1 against the definition on the planes the pack wrote, sym = 0 and 1"""
    raw = di.case_input(F)[2][:R * F]
    p, rref, planes, Npad = dev_pack(ctx, raw, None)
    a4, w4 = planes_from(p, F)
    w2 = (w4 ** 2).sum(axis=1).T                                           # (V, R)
    for sym in (0, 1):
        P0, dP0, C, dC, ws = dev_ct_pair(ctx, planes, Npad, V, R, F, PAIRS, sym, 1)
        P0r, dP0r, Cr, dCr, _ = core_pair(a4, w4, PAIRS, sym)
        report('direct pairs mode 1 sym=%d' % sym, F, di.PAIR_NAMES, C, dC, Cr, dCr)
        assert ci.close(C, dC, Cr, dCr, R, ci.BAR_F64) and di.close_p0(P0, dP0, P0r, dP0r, ci.BAR_F64)
        assert relerr(ws[:, :, 0], w2[PAIRS[:, 0]]) <= 1e-12 and relerr(ws[:, :, 1], w2[PAIRS[:, 1]]) <= 1e-12


@pytest.mark.parametrize('sym', [0, 1])
@pytest.mark.parametrize('F', PAIR_DIRECT)
def test_direct_pairs_float32(ctx, F, sym):
    ref = di.reference_pairs(F, sym)
    assert F <= ctx.ct_dipolar_cross_max_frames() and F < ctx.ct_dipolar_cross_long_min_frames
    with options(ctx):
        got = hostct.calculate_Ct_dipolar_cross(raw4(F), PAIRS, symmetric=bool(sym), ctx=ctx, mode=0)
        check_pairs('direct pairs mode 0 sym=%d' % sym, F, got, ref, ci.NORTH_STAR)
        auto = hostct.calculate_Ct_dipolar(raw4(F), ctx=ctx, mode=0)
        check_pair_identities('direct pairs', F, sym, got, ref, auto, ci.NORTH_STAR)
        assert same_bytes(got, hostct.calculate_Ct_dipolar_cross(raw4(F), PAIRS, symmetric=bool(sym), ctx=ctx, mode=0))
        if F == 257 and sym:
            u, d, _ = di.case_input(F)
            alt = hostct.calculate_Ct_dipolar_cross(u[:R * F].reshape(R, F, V, 3), PAIRS, dist=d[:R * F].reshape(R, F, V), ctx=ctx, mode=0)
            check_pairs('direct pairs mode 0, dist given', F, alt, di.reference_pairs(F, 1, 'dist'), ci.NORTH_STAR)


# ---- the blocked autocorrelation form -----------------------------------------------------------------------------------------------------------
def blocked_auto_on_planes(ctx, F, raw, starts=None):
    """mode 1 and mode 0 of sr_ct_dipolar_long_f32_dev on the planes the pack wrote against the definition on those planes: 1e-12 and
    the north star"""
    import torch
    p, rref, planes, Npad = dev_pack(ctx, raw, None)
    a4, w4 = planes_from(p, F, starts)
    Cr, dCr, w1, w2 = fft_core(a4, w4)
    L = F // 2
    Ct = torch.empty((L, V), device='cuda', dtype=torch.float64)
    dCt = torch.empty((L, V), device='cuda', dtype=torch.float64)
    wm = torch.empty((V, 2), device='cuda', dtype=torch.float64)
    for mode, bar in ((1, ci.BAR_F64), (0, ci.NORTH_STAR)):
        ctx.ct_dipolar_long_dev(planes.data_ptr(), Npad, V, R, F, Ct.data_ptr(), dCt.data_ptr(), wm.data_ptr(), chunk_start=starts, mode=mode)
        ctx.sync()
        C, dC, w = Ct.cpu().numpy(), dCt.cpu().numpy(), wm.cpu().numpy()
        report('blocked auto mode %d on the planes' % mode, F, SERIES, C, dC, Cr, dCr)
        assert ci.close(C, dC, Cr, dCr, R, bar), mode
        assert relerr(w[:, 0], w1) <= 1e-12 and relerr(w[:, 1], w2) <= 1e-12


@pytest.mark.parametrize('F,minf', AUTO_BLOCKED)
def test_blocked_autocorrelation(ctx, F, minf):
    """5462 with "ct_dipolar_long_min_frames" lowered, 10017 (the first length the direct kernel refuses) and 12289 (one sample in the
    last block) through the default dispatch.  Bar 1: the north star.  Bar 2: 4 x the emulation's error per series."""
    ref = di.reference_auto(F)
    b2, emu = di.bar2(F)
    with options(ctx, ct_dipolar_long_min_frames=minf):
        assert F >= ctx.ct_dipolar_long_min_frames
        got = hostct.calculate_Ct_dipolar(raw4(F), ctx=ctx, mode=0)
        check_auto('blocked auto mode 0', F, got, ref, ci.NORTH_STAR, b2, emu)
        assert same_bytes(got, hostct.calculate_Ct_dipolar(raw4(F), ctx=ctx, mode=0))
        check_const_series(ctx, 'blocked auto', F, got)
        blocked_auto_on_planes(ctx, F, di.case_input(F)[2][:R * F])
    if F == 5462:
        with options(ctx):
            direct = hostct.calculate_Ct_dipolar(raw4(F), ctx=ctx, mode=0)
        check_auto('direct auto mode 0', F, direct, ref, ci.NORTH_STAR)
        eC, eD = ci.errors(got[0], got[1], direct[0], direct[1], R)
        print('[dipolar mobile] blocked against direct F=%d  |dC|/scale   %s' % (F, fmt(SERIES, eC)))
        assert ci.close(got[0], got[1], direct[0], direct[1], R, ci.NORTH_STAR)
        assert got[0].tobytes() != direct[0].tobytes()                     # two kernels: the option took the blocked form


def test_blocked_autocorrelation_with_an_odd_chunk_start(ctx):
    """chunk starts 0, F + 4 (odd) and 2 F + 11 at F = 10017: the unaligned load path; r_ref runs over all frames held"""
    F = 10017
    raw = di.case_input(F)[2]
    starts = di.odd_starts(F)
    assert starts[1] % 2 == 1 and starts[2] + F <= raw.shape[0]
    ref = di.reference_auto(F, 'raw', starts)
    b2, emu = di.bar2(F, starts)
    with options(ctx):
        with ctx.vectors(V, raw.shape[0]) as rv:
            rv.append(raw)
            got = hostct.calculate_Ct_dipolar_resident(rv, R, F, chunk_start=starts)
        check_auto('blocked auto mode 0, odd start', F, got, ref, ci.NORTH_STAR, b2, emu)
        blocked_auto_on_planes(ctx, F, raw, starts)


# ---- the blocked pair form ------------------------------------------------------------------------------------------------------------------
def blocked_pairs_on_planes(ctx, F, raw, sym):
    import torch
    p, rref, planes, Npad = dev_pack(ctx, raw, None)
    a4, w4 = planes_from(p, F)
    ref = fft_cross_core(a4, w4, PAIRS, sym)
    L, nP = F // 2, len(PAIRS)
    P0 = torch.empty((2, nP), device='cuda', dtype=torch.float64)
    Ct = torch.empty((L, nP), device='cuda', dtype=torch.float64)
    dCt = torch.empty((L, nP), device='cuda', dtype=torch.float64)
    ws = torch.empty((nP, R, 2), device='cuda', dtype=torch.float64)
    w2 = (w4 ** 2).sum(axis=1)                                             # (R, V)
    for mode, bar in ((1, ci.BAR_F64), (0, ci.NORTH_STAR)):
        ctx.ct_dipolar_cross_long_dev(planes.data_ptr(), Npad, V, R, F, PAIRS, P0[0].data_ptr(), Ct.data_ptr(), dCt.data_ptr(), ws.data_ptr(),
                                      sym=sym, mode=mode, dP0_ptr=P0[1].data_ptr())
        ctx.sync()
        P, C, dC, w = P0.cpu().numpy(), Ct.cpu().numpy(), dCt.cpu().numpy(), ws.cpu().numpy()
        report('blocked pairs mode %d sym=%d on the planes' % (mode, sym), F, di.PAIR_NAMES, C, dC, ref[2], ref[3])
        assert ci.close(C, dC, ref[2], ref[3], R, bar) and di.close_p0(P[0], P[1], ref[0], ref[1], bar), mode
        assert relerr(w[:, :, 0], w2[:, PAIRS[:, 0]].T) <= 1e-12 and relerr(w[:, :, 1], w2[:, PAIRS[:, 1]].T) <= 1e-12


@pytest.mark.parametrize('sym', [0, 1])
@pytest.mark.parametrize('F,minf', PAIR_BLOCKED)
def test_blocked_pairs(ctx, F, minf, sym):
    """4097 with "ct_dipolar_cross_long_min_frames" lowered, 4897 (the first length the direct pair kernel refuses) and 8193 (one sample
    in the third block) through the default dispatch.  Bar 2 of a pair: the larger of its two series' bars."""
    ref = di.reference_pairs(F, sym)
    b2s, _ = di.bar2(F)
    b2 = np.maximum(b2s[PAIRS[:, 0]], b2s[PAIRS[:, 1]])
    with options(ctx, ct_dipolar_cross_long_min_frames=minf):
        assert F >= ctx.ct_dipolar_cross_long_min_frames
        got = hostct.calculate_Ct_dipolar_cross(raw4(F), PAIRS, symmetric=bool(sym), ctx=ctx, mode=0)
        check_pairs('blocked pairs mode 0 sym=%d' % sym, F, got, ref, ci.NORTH_STAR, b2)
        assert same_bytes(got, hostct.calculate_Ct_dipolar_cross(raw4(F), PAIRS, symmetric=bool(sym), ctx=ctx, mode=0))
        auto = hostct.calculate_Ct_dipolar(raw4(F), ctx=ctx, mode=0)           # these lengths: the direct autocorrelation form
        check_pair_identities('blocked pairs', F, sym, got, ref, auto, ci.NORTH_STAR)
        blocked_pairs_on_planes(ctx, F, di.case_input(F)[2][:R * F], sym)
    with options(ctx):
        if F == 4097:
            direct = hostct.calculate_Ct_dipolar_cross(raw4(F), PAIRS, symmetric=bool(sym), ctx=ctx, mode=0)
            check_pairs('direct pairs mode 0 sym=%d' % sym, F, direct, ref, ci.NORTH_STAR)
            eC, eD = ci.errors(got[2], got[3], direct[2], direct[3], R)
            print('[dipolar mobile] blocked against direct F=%d sym=%d  |dC|/scale   %s' % (F, sym, fmt(di.PAIR_NAMES, eC)))
            assert ci.close(got[2], got[3], direct[2], direct[3], R, ci.NORTH_STAR)
            assert di.close_p0(got[0], got[1], direct[0], direct[1], ci.NORTH_STAR)
            assert got[2].tobytes() != direct[2].tobytes()                 # two kernels: the option took the blocked form
