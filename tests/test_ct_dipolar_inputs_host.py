"""
CPU tests (no GPU) of tests/ct_dipolar_inputs.py: the conditions that make tests/test_gpu_ct_dipolar_mobile.py mean something, asserted
on the very arrays the GPU tests use (ct_dipolar_inputs.CASES), so a changed generator or seed cannot quietly turn the inputs back
into easy ones.  The seeds of CASES were chosen by scanning 1, 2, ... for the first that meets every condition below at that length
(128: 361 and 257: 64 -- a log-normal walk of correlation time 100 frames rarely spans the factor 1000 in w within 400 or 800 frames;
every other length: 1, 2 or 4).

What holds from which length on: the conditions on the distances themselves (WIDE, SPIKE, ANGLE) at every length; a sign change of the
reference C_dd and a value below 1e-3 in every chunk, the chunk-to-chunk spread of a WIDE series and the pairs' P0 from F = 682 on
(ct_inputs.MOBILE_FROM: 128 and 257 have 64 and 128 lags); a chunk without a contact beside one with an episode of 64 frames from
F = 1000 on.  The per-chunk C_dd of these conditions comes from the FFT oracle, which test_fft_oracles_agree_on_the_mixed_input holds
to 1e-12 of the lag-by-lag one on this input.

The pair that shares its direction with series 1 under an independent CONTACT distance has P0 = <w_i w_j> / sqrt(<w_i^2> <w_j^2>), the
cosine of two independent heavy-tailed weights: 0.04 .. 0.55 here, not near 1.  The pairs (i, i) are the ones with P0 > 0.5.
"""
import hashlib

import numpy as np
import pytest

import ct_dipolar_inputs as di
import ct_inputs as ci
from test_gpu_ct_dipolar import oracle_dipolar
from test_gpu_ct_dipolar_cross import oracle_dcross

R = di.R
SHA = {
    'mild': 'c940364ca247ebd80f91c2f4a21c844ed1a9ee6a1cac5326772eabe778b83924',
    'wide': '4f987fbc3ebd9c1f61ecf35864fe198fd4415eb5a3404accf447d14aba4b6ddc',
    'contact': '8c8d1ea9417dfee74f9799d19b09e3c6a72bf8e96c3258abef100475e6be1bb6',
    'angle': '57b24d2f92338de2980ca3833a7cbf5ae8011d006ecb7f9ca26fdbac9a352709',
    'spike': '1e774026d06a1cdad49e0057585d1a7455c77881c50a13ee94bfcc2e9d88b5a7',
    'const': '12f9eb279727de046bb559389f6e734da3cf5233dd1310e4109595ffe511f33a',
    'mixed u': 'a484cb06df80aa1674b8dd01ec5c487e139a184e721e36d36119dbef7f1c4fd1',
    'mixed dist': 'f9928f38261d47e7a9d5548f454486772126e7c0b9e80e294a0130fb4db2a821',
    'mixed raw': 'ed6f49fdc22afa5e74acc92e2f85e788bff37c2f03d25970fe57eff49f92200d',
}
# max_t |emulate_dipolar_f32 - oracle| / scale of C_dd on one chunk of four walk.02 series per distance process: (F, M) -> mild, wide,
# contact, angle, spike, const
EMULATION = {(684, 2048): (1.2e-7, 1.1e-7, 1.4e-7, 9.7e-8, 7.6e-8, 1.3e-7), (2731, 8192): (1.8e-7, 1.2e-7, 1.0e-7, 1.8e-7, 5.3e-8, 1.9e-7)}
EMU_SEED = 11


def small_arrays():
    N = 300
    out = {name: di.process(kind, N, 2, 5) for kind, name in enumerate(di.PROCESSES)}
    u, d, raw = di.mixed(N, 5, 100)
    out.update({'mixed u': u, 'mixed dist': d, 'mixed raw': raw})
    return out


def test_generators_are_bit_reproducible():
    for name, a in small_arrays().items():
        assert a.dtype == np.float32 and a.shape[0] == 300 and not a.flags.writeable and np.all(a == a), name
        assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == SHA[name], name
    assert di.mixed(300, 5, 100) is di.mixed(300, 5, 100) and di.process(di.WIDE, 300, 2, 5) is di.process(di.WIDE, 300, 2, 5)      # cached
    x = np.linspace(-4.0, 4.0, 801)
    assert np.max(np.abs(di._exp64(x) / np.exp(x) - 1.0)) < 1e-12
    # the mixed input is what its docstring says: unit directions, raw = float32(u dist), series 8 repeats the direction of series 1
    u, d, raw = di.mixed(300, 5, 100)
    assert np.max(np.abs((u.astype(np.float64) ** 2).sum(-1) - 1.0)) < ci.UNIT_TOL
    assert np.array_equal(raw, (u.astype(np.float64) * d.astype(np.float64)[..., None]).astype(np.float32))
    assert np.array_equal(u[:, di.SHARED_CONTACT], u[:, di.SLOW_WIDE]) and len(np.unique(d[:, di.SLOW_CONST])) == 1
    assert not np.array_equal(d[:, di.SHARED_CONTACT], d[:, di.JUMP_CONTACT])


def test_the_pair_list_holds_what_the_cross_tests_need():
    P = di.PAIRS
    assert tuple(P[di.P_II_WIDE]) == (di.SLOW_WIDE,) * 2 and tuple(P[di.P_II_CONTACT]) == (di.JUMP_CONTACT,) * 2
    assert tuple(P[di.P_IJ]) == tuple(P[di.P_JI][::-1]) == tuple(P[di.P_REPEAT]) == (di.SLOW_WIDE, di.FAST_WIDE)
    assert tuple(P[di.P_SHARED]) == (di.SLOW_WIDE, di.SHARED_CONTACT) and tuple(P[di.P_INDEP]) == (di.JUMP_CONTACT, di.WHITE_CONTACT)
    assert len(di.PAIR_NAMES) == len(P) and len(di.SERIES) == di.NSER == 9


@pytest.mark.parametrize('F', sorted(di.CASES))
def test_inputs_stay_hard(F):
    tables = [None, di.odd_starts(F)] if F == 10017 else [None]
    u, d, raw = di.case_input(F)
    assert raw.shape == (R * F + di.TAIL, 9, 3) and di.odd_starts(F)[2] + F <= raw.shape[0]
    for starts in tables:
        f = di.figures(F, di.CASES[F], starts)
        print('\n[dipolar inputs] F=%d%s' % (F, '' if starts is None else ' odd starts'))
        for k, val in f.items():
            print('[dipolar inputs]   %s: %s' % (k, np.array2string(np.asarray(val), precision=3, max_line_width=200).replace('\n', ' ')))
        assert di.failed(f, F) == []
        # the same conditions, spelled out
        assert np.all(f['wide_min_w'] < 1e-3) and f['wide_chunk_ratio'] >= 4.0
        assert f['spike_frames_w1'] == 1 and f['spike_other_max_w'] < 1e-3 and f['angle_corr'] > 0.9
        if F >= di.CONTACT_FROM:
            assert f['contact_chunks_without'] >= 1 and f['contact_longest_episode'] >= 64
        if F >= di.MOBILE_FROM:
            assert np.all(f['mobile_sign_change']) and np.all(f['mobile_min_abs_C'] < 1e-3)
            assert np.max(f['wide_max_dC']) > 0.1
            assert np.min(np.abs(f['P0'])) < 0.05 and np.max(f['P0']) > 0.5
            assert abs(f['P0'][di.P_INDEP]) < 0.05 and f['P0'][di.P_SHARED] > 0.02
    # the MILD control stays what make_pairs is: w within a factor 20 at every length
    a, w, _ = di.planes(F)
    assert w[:, di.WOB_MILD].min() > 0.05


def test_fft_oracles_agree_on_the_mixed_input():
    """the FFT oracles of the long chunks against the lag-by-lag oracles at 16 probed lags, F = 5462, both forms, on the mixed input"""
    F = 5462
    u, d, raw = di.case_input(F)
    raw = raw[:R * F]
    lags = np.unique(np.linspace(1, F // 2, 16).astype(int))
    assert len(lags) == 16
    fa = di.reference_auto(F)
    la = oracle_dipolar(raw, None, R, F, lags=lags)
    scale = ci.scale_of(fa[0])
    print('\n[dipolar inputs] FFT against lag-by-lag, auto: C %.1e dC %.1e' % (np.max(np.abs(fa[0][lags - 1] - la[0]) / scale),
                                                                              np.max(np.abs(fa[1][lags - 1] - la[1]) / scale)))
    assert np.all(np.abs(fa[0][lags - 1] - la[0]) <= 1e-12 * scale) and np.all(np.abs(fa[1][lags - 1] - la[1]) <= 1e-12 * scale)
    for x, y in zip(fa[2:], la[2:]):
        assert np.max(np.abs(x / y - 1.0)) <= 1e-12
    for sym in (0, 1):
        fp = di.reference_pairs(F, sym)
        lp = oracle_dcross(raw, None, di.PAIRS, sym, R, F, lags=lags)
        scale = ci.scale_of(np.vstack([fp[2], fp[0][None]]))
        assert np.all(np.abs(fp[2][lags - 1] - lp[2]) <= 1e-12 * scale) and np.all(np.abs(fp[3][lags - 1] - lp[3]) <= 1e-12 * scale)
        assert np.all(np.abs(fp[0] - lp[0]) <= 1e-12 * scale) and np.all(np.abs(fp[1] - lp[1]) <= 1e-12 * scale)


def emulation_chunk(kind, F):
    """a4, w4 float32 (1, F, 4, .) of four walk.02 directions under one distance process, and the oracle of that chunk"""
    u = ci.walk(F, 4, EMU_SEED, ci.STEP_SLOW)
    d = di.process(kind, F, 4, EMU_SEED, F)
    a, w, _ = di.planes_of(u, d)
    a32, w32 = di.f32_planes(a, w)
    Cr, dCr = di.oracle_dipolar(u, d, 1, F)[:2]
    return a32[None], w32[None], Cr, dCr


def test_emulation_is_pinned():
    """emulate_dipolar_f32 against the oracle, one chunk per distance process: the figures of the table within a factor 2, so the
    regression bar of the blocked forms hangs on a pinned emulation"""
    for (F, M), table in EMULATION.items():
        for kind, want in enumerate(table):
            a4, w4, Cr, dCr = emulation_chunk(kind, F)
            Ce, dCe = di.emulate_dipolar_f32(a4, M, w4)
            got = np.max(np.abs(Ce - Cr) / ci.scale_of(Cr)[None])
            print('[emulate_dipolar_f32] F=%d M=%d %s: %.2e (table %.1e)' % (F, M, di.PROCESSES[kind], got, want))
            assert 0.5 * want <= got <= 2.0 * want, (F, di.PROCESSES[kind], got, want)
            assert np.all(np.isnan(dCe)) and got < ci.NORTH_STAR
            # the w plane and |a|^2 agree to the rounding of the pack: the normaliser does not care which it takes
            Ca, _ = di.emulate_dipolar_f32(a4, M)
            assert np.max(np.abs(Ca - Ce)) < 1e-7


def test_emulation_needs_every_mean_restored():
    """one of the five signals' means left out: off by more than 1e-4 on a WIDE series, whichever signal it is"""
    F, M = 684, 2048
    a4, w4, Cr, dCr = emulation_chunk(di.WIDE, F)
    for c in range(5):
        restore = tuple(k != c for k in range(5))
        Ce, _ = di.emulate_dipolar_f32(a4, M, w4, restore=restore)
        err = np.max(np.abs(Ce - Cr), axis=0)
        print('[emulate_dipolar_f32] mean of signal %d not restored: %s' % (c, ' '.join('%.1e' % e for e in err)))
        assert np.max(err) > 1e-4, c


def test_close_accepts_and_rejects_at_the_element_nearest_zero():
    F = 257
    Cr, dCr = di.reference_auto(F)[:2]
    scale = ci.scale_of(Cr)
    assert np.all(scale == 1.0)
    for bar in (ci.NORTH_STAR, ci.BAR_F64, np.full(9, 1e-7)):
        b = np.ones(9) * bar
        assert ci.close(Cr, dCr, Cr, dCr, R, bar)
        for k in (di.FAST_WIDE, di.WHITE_CONTACT, di.FAST_SPIKE):
            lag = int(np.argmin(np.abs(Cr[:, k])))                      # the element nearest zero: the bar does not shrink with it
            assert abs(Cr[lag, k]) < 1e-2
            for sign in (1.0, -1.0):
                C = Cr.copy()
                C[lag, k] += sign * 2.0 * b[k] * scale[k]
                assert not ci.close(C, dCr, Cr, dCr, R, bar)
                C[lag, k] = Cr[lag, k] + sign * 0.5 * b[k] * scale[k]
                assert ci.close(C, dCr, Cr, dCr, R, bar)
    P0, dP0 = di.reference_pairs(F, 1)[:2]
    k = di.P_INDEP
    for sign in (1.0, -1.0):
        P = P0.copy()
        P[k] += sign * 2e-6
        assert not di.close_p0(P, dP0, P0, dP0, ci.NORTH_STAR)
        P[k] = P0[k] + sign * 0.5e-6
        assert di.close_p0(P, dP0, P0, dP0, ci.NORTH_STAR)
    bad = P0.copy()
    bad[0] = np.nan
    assert not di.close_p0(bad, dP0, P0, dP0, ci.NORTH_STAR) and not di.close_p0(P0, bad, P0, dP0, ci.NORTH_STAR)


def test_bar2_is_four_times_the_emulation():
    for F in (5462, 10017):
        for starts in ([None, di.odd_starts(F)] if F == 10017 else [None]):
            b, emu = di.bar2(F, starts)
            assert b.shape == emu.shape == (9,) and np.all(b <= ci.NORTH_STAR)
            assert np.array_equal(b, np.minimum(ci.NORTH_STAR, ci.EMU_FACTOR * emu))
            assert np.all(emu > 2e-9) and np.all(emu < 2.5e-7)            # no series is exact for the emulation: none takes a floor
