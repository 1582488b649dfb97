"""
GPU tests (marker gpu) of kernel 1, C(t), and of the pair kernels on MOBILE vectors: every formulation of the dispatch table of
csrc/sr_ct.hip on the eight series of ct_inputs.mixed -- the wobbling series of synth_vectors beside series that tumble, jump, are
uncorrelated, are not unit vectors, hold zero vectors, flip sign -- against the plain-C float64 oracle (oracle/libsr_oracle.so), with
bars that are ABSOLUTE at the scale of C(0) (ct_inputs.close; C(t) of these series passes through zero, where a bar relative to the
element says nothing).  The conditions that make the inputs mobile are asserted without a GPU in tests/test_ct_inputs_host.py.

Every test asserts first, by sr_ct_formulation (the function the library itself switches on), that the options it sets select the
formulation it means to run, and prints its worst |dC| / scale and |d dC| (sqrt(R) - 1) / scale per series; docs/EXPERIMENTS.md
section 27 is filled from those prints.

Bars (ct_inputs):
  * float64 formulations (mode 1, k_ct_fft, k_ct_rfft): 1e-12, the figure the existing tests assert for them, here absolute;
  * direct float32 kernel k_ct_palmer: 1e-6, the north star of BASELINE.json and the RTOL of tests/test_gpu_parity.py;
  * float32 transforms (k_ct_rfft32, the blocked k_ctl_*, sr_ct_cross_long): BOTH 1e-6 and, per series, 4 x the error of an
    independent float32 implementation (ct_inputs.emulate_f32: scipy's float32 transforms, means restored in float64) on the same
    chunks, never more than 1e-6 (ct_inputs.bar2_of; on the antipodal series alone, where the emulation is exact, the figure it
    multiplies is at least 2^-24).  The factor 4 covers the difference between
    pocketfft's transforms and the kernels' radix-16 register steps with table twiddles and float32 e[j]; it is not a measured
    figure of the kernels.  For the blocked kernels the emulation is ONE transform of the whole chunk at the next power of two.
"""
import contextlib

import numpy as np
import pytest

import ct_inputs as ci
from ct_inputs import ANTIPODAL, JUMP, SCALED, WALK_SLOW, WHITE, WOBBLE
from spinrelax_amd import _lib
from spinrelax_amd import ct as hostct
import sr_oracle as o
from test_gpu_ct_cross import oracle_cross

pytestmark = pytest.mark.gpu

REFUSED, DIRECT, FFT64, RFFT64, RFFT32, BLOCKED = range(6)          # SR_CT_* of include/spinrelax_hip.h
NAMES = ('refused', 'k_ct_palmer', 'k_ct_fft', 'k_ct_rfft', 'k_ct_rfft32', 'k_ctl_*')
DEFAULTS = dict(ct_fft=3, ct_traceless=0, ct_long_min_frames=16384, ct_cross_long_min_frames=6625)


@pytest.fixture(scope='module')
def ctx():
    from spinrelax_amd.hip import Context
    c = Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def options(ctx, **kw):
    """EVERY option of DEFAULTS is set, to kw's value or to its default (the library has no call that reads an option back): what runs
    inside does not depend on what an earlier test left behind, and the defaults are back afterwards"""
    assert set(kw) <= set(DEFAULTS)
    try:
        for k, val in {**DEFAULTS, **kw}.items():
            ctx.set_option(k, val)
        yield
    finally:
        for k, val in DEFAULTS.items():
            ctx.set_option(k, val)


def formulation(ctx, opts, mode, F):
    """what sr_ct_palmer_sums_f32_dev switches on inside options(ctx, **opts) (sr_lds_limit: the larger of the two LDS sizes of the
    device)"""
    full = {**DEFAULTS, **opts}
    lds = max(ctx.device_info()['lds_per_cu'], 64 * 1024)
    return _lib.load().sr_ct_formulation(full['ct_fft'], full['ct_long_min_frames'], mode, F, lds)


def run(ctx, form, opts, mode, vecs, R, F, **kw):
    assert formulation(ctx, opts, mode, F) == form, (NAMES[form], opts, mode, F)
    with options(ctx, **opts):
        return ctx.ct_palmer(vecs, R, F, mode=mode, **kw)


def report(tag, F, R, Ct, dCt, Cr, dCr, emu=None):
    eC, eD = ci.errors(Ct, dCt, Cr, dCr, R)
    print('\n[mobile] %s F=%d R=%d  |dC|/scale   %s' % (tag, F, R, ' '.join('%s %.1e' % kv for kv in zip(ci.KINDS, eC))))
    print('[mobile] %s F=%d R=%d  |d dC|(sqrt(R)-1)/scale   %s' % (tag, F, R, ' '.join('%s %.1e' % kv for kv in zip(ci.KINDS, eD))))
    if emu is not None:
        print('[mobile] %s F=%d R=%d  emulation |dC|/scale   %s' % (tag, F, R, ' '.join('%s %.1e' % kv for kv in zip(ci.KINDS, emu))))
    return eC, eD


def check_mixed(ctx, tag, form, opts, mode, F, bar, f32_transform=False):
    vecs, R, Cr, dCr = ci.case(F)
    Ct, dCt = run(ctx, form, opts, mode, vecs, R, F)
    assert Ct.shape == dCt.shape == (F // 2, 8)
    b2, emu = ci.bar2(F) if f32_transform else (None, None)
    report(tag, F, R, Ct, dCt, Cr, dCr, emu)
    assert ci.close(Ct, dCt, Cr, dCr, R, bar), (tag, F)
    if f32_transform:
        assert ci.close(Ct, dCt, Cr, dCr, R, b2), (tag, F, 'bar 2', b2)


# ---- one test per formulation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,opts', [(7, {}), (255, {}), (257, {}), (682, {}), (683, {}), (1000, {'ct_fft': 0})])
def test_direct_float32(ctx, F, opts):
    """k_ct_palmer: chosen by need = F + L <= 1024 (682: need 1023, 683: need 1024, the last) or by ct_fft = 0; one lag block and less,
    two and three lag blocks, the float64 tail path of the lags that fill no block"""
    check_mixed(ctx, 'direct f32', DIRECT, opts, 0, F, ci.NORTH_STAR)


@pytest.mark.parametrize('F', [257, 1000])
def test_direct_float64(ctx, F):
    check_mixed(ctx, 'direct f64', DIRECT, {}, 1, F, ci.BAR_F64)


@pytest.mark.parametrize('F', [684, 1366, 2731])
def test_complex_float64_transforms(ctx, F):
    """k_ct_fft (ct_fft = 1) with 2048, 4096 and 8192 points; 684 is its first length (683 has need = 1024 and stays with k_ct_palmer
    whatever ct_fft says: test_direct_float32)"""
    check_mixed(ctx, 'fft64', FFT64, {'ct_fft': 1}, 0, F, ci.BAR_F64)


@pytest.mark.parametrize('traceless', [0, 1])
@pytest.mark.parametrize('F', [4096, 3001, 4097])
def test_real_float64_transforms(ctx, F, traceless):
    """k_ct_rfft (ct_fft = 2): N1 = 12 full and masked, N1 = 16; six signals, and five with the trace term from prefix sums"""
    check_mixed(ctx, 'rfft64 traceless=%d' % traceless, RFFT64, {'ct_fft': 2, 'ct_traceless': traceless}, 0, F, ci.BAR_F64)


@pytest.mark.parametrize('F,opts', [(684, {'ct_fft': 4}), (1365, {'ct_fft': 4}), (1366, {'ct_fft': 4}), (2730, {'ct_fft': 4}),
                                    (2731, {'ct_fft': 4}), (4095, {}), (4096, {}), (4097, {}), (5461, {})])
def test_float32_transforms(ctx, F, opts):
    """k_ct_rfft32 with N1 = 4 (684, 1365), 8 (1366, 2730, 2731), 12 (4095; 4096: the FULL instantiation) and 16 (4097, 5461): by
    ct_fft = 4 below need = 4096 and by the default dispatch above"""
    check_mixed(ctx, 'rfft32', RFFT32, opts, 0, F, ci.NORTH_STAR, f32_transform=True)


@pytest.mark.parametrize('F,opts', [(5462, {'ct_long_min_frames': 5462}), (8193, {'ct_long_min_frames': 5462}),
                                    (12289, {'ct_long_min_frames': 5462}), (16384, {})])
def test_blocked_float32_transforms(ctx, F, opts):
    """k_ctl_*: the seam inside the second (5462) and third (8193) block, four blocks and nd = 2 (12289), and the first length of the
    default dispatch"""
    check_mixed(ctx, 'blocked', BLOCKED, opts, 0, F, ci.NORTH_STAR, f32_transform=True)


# ---- chunk starts, shards ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,form,opts', [(4096, RFFT32, {}), (8193, BLOCKED, {'ct_long_min_frames': 5462})])
def test_odd_chunk_starts(ctx, F, form, opts):
    """two "files", the first of odd length (ct_inputs.chunk_start_case): the third chunk starts at an odd frame (32-bit loads), the
    tails are dropped per file"""
    cat, starts, R, v4, Cr, dCr = ci.chunk_start_case(F)
    n = 2 * F + 1
    cat2, starts2, R2 = hostct.concat_with_chunk_starts([cat[:n], cat[n:]], F)
    assert R2 == R == 3 and np.array_equal(starts2, starts) and starts[2] % 2 == 1 and np.array_equal(cat2, cat)
    Ct, dCt = run(ctx, form, opts, 0, cat, R, F, chunk_start=starts)
    b2, emu = ci.bar2_of(v4, Cr, dCr)
    report('chunk starts ' + NAMES[form], F, R, Ct, dCt, Cr, dCr, emu)
    assert ci.close(Ct, dCt, Cr, dCr, R, ci.NORTH_STAR)
    assert ci.close(Ct, dCt, Cr, dCr, R, b2), ('bar 2', b2)


@pytest.mark.parametrize('F,form,opts', [(257, DIRECT, {}), (1366, FFT64, {'ct_fft': 1}), (4097, RFFT64, {'ct_fft': 2}), (4096, RFFT32, {}),
                                         (5462, BLOCKED, {'ct_long_min_frames': 5462})])
def test_shard_equals_full_run(ctx, F, form, opts):
    vecs, R = ci.case_input(F)
    full, dfull = run(ctx, form, opts, 0, vecs, R, F)
    part, dpart = run(ctx, form, opts, 0, vecs, R, F, v0=2, nV=5)
    np.testing.assert_array_equal(part, full[:, 2:7])
    np.testing.assert_array_equal(dpart, dfull[:, 2:7])


# ---- properties ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,form,bar', [(1000, FFT64, ci.BAR_F64), (4096, RFFT32, ci.NORTH_STAR)])
def test_properties_on_a_tumbling_series(ctx, F, form, bar):
    """walk(step 0.15) through the default dispatch: time reversal inside every chunk, a fixed rotation of every frame (inputs
    re-rounded to float32: 5e-7, the allowance of test_ct_size_independent_properties), -0.5 <= C <= 1"""
    R, V = 3, 4
    vecs = ci.walk(R * F, V, 3, ci.STEP_FAST)
    Ct, dCt = run(ctx, form, {}, 0, vecs, R, F)
    scale = ci.scale_of(Ct)[None, :]
    rev = np.ascontiguousarray(vecs.reshape(R, F, V, 3)[:, ::-1].reshape(R * F, V, 3))
    Cv, _ = run(ctx, form, {}, 0, rev, R, F)
    rot = o.rotate_vector_simd(vecs, np.array([0.5, -0.5, 0.5, 0.5])).astype(np.float32)
    Co, _ = run(ctx, form, {}, 0, rot, R, F)
    print('\n[mobile] properties %s F=%d: time reversal %.1e, rotation %.1e, min C %.4f max C %.4f'
          % (NAMES[form], F, np.max(np.abs(Cv - Ct) / scale), np.max(np.abs(Co - Ct) / scale), Ct.min(), Ct.max()))
    assert np.all(np.abs(Cv - Ct) <= bar * scale)
    assert np.all(np.abs(Co - Ct) <= 5e-7 * scale)
    assert Ct.min() >= -0.5 - bar and Ct.max() <= 1.0 + bar
    assert Ct.min() < 0.0 < Ct.max()


# ---- known answers -----------------------------------------------------------------------------------------------------------------------------
KNOWN = [('direct f32', DIRECT, {}, 0, 257, ci.NORTH_STAR), ('direct f64', DIRECT, {}, 1, 257, ci.BAR_F64),
         ('fft64', FFT64, {'ct_fft': 1}, 0, 684, ci.BAR_F64),
         ('rfft64', RFFT64, {'ct_fft': 2}, 0, 3001, ci.BAR_F64), ('rfft64 traceless', RFFT64, {'ct_fft': 2, 'ct_traceless': 1}, 0, 3001, ci.BAR_F64),
         ('rfft32', RFFT32, {}, 0, 4097, ci.NORTH_STAR), ('blocked', BLOCKED, {'ct_long_min_frames': 5462}, 0, 5462, ci.NORTH_STAR)]


@pytest.mark.parametrize('tag,form,opts,mode,F,bar', KNOWN, ids=[k[0].replace(' ', '_') for k in KNOWN])
def test_known_answers(ctx, tag, form, opts, mode, F, bar):
    """Series whose C(t) needs no oracle, R = 2, three trailing frames.
    antipodal, u_0 = z: every product of two components is 0 or 1, every mean-removed signal vanishes, C(t) = 1 and dC(t) = 0 to the
    4e-15 of the constant-vector tests, in every formulation.  antipodal, u_0 on no axis: C(t) = 1.5 |u_0|^4 - 0.5; the products are
    constant, but the float32 transforms round x^2, y^2, z^2 before they combine them into the first two signals and hold e[j] in
    float32, and the direct kernel rounds every dot product -- roundings that add up on a constant series instead of averaging out
    (measured 1.3e-8 and 9.5e-8): the formulation's bar.  alternating and three_site (exactly representable inputs, C = -0.5 | 1): the
    formulation's bar.  The float32 transforms also meet bar 2 on all three, the emulation run on the same series (off the axes it is
    exact and the 2^-24 of the antipodal series applies; on the periodic series it is off by 2e-7 and 4e-7 like the kernels)."""
    R = 2
    N = R * F + ci.TAIL
    L = F // 2
    anti = ci.antipodal(N, 9)
    Ct, dCt = run(ctx, form, opts, mode, anti, R, F)
    want = np.broadcast_to(ci.antipodal_answer(anti)[None, :], (L, 2))
    err = np.max(np.abs(Ct - want), axis=0)
    print('\n[mobile] known answers %s F=%d: antipodal z %.1e (dC %.1e), off-axis %.1e (dC %.1e)'
          % (tag, F, err[0], np.max(np.abs(dCt[:, 0])), err[1], np.max(np.abs(dCt[:, 1]))))
    assert err[0] <= ci.BAR_EXACT and np.max(np.abs(dCt[:, 0])) <= ci.BAR_EXACT
    assert ci.close(Ct[:, 1:], dCt[:, 1:], want[:, 1:], np.zeros((L, 1)), R, bar)
    f32_transform = form in (RFFT32, BLOCKED)
    if f32_transform:
        b2, emu = ci.bar2_of(anti[:R * F].reshape(R, F, 2, 3), want, np.zeros((L, 2)), floor_columns=(0, 1))
        print('[mobile] known answers %s F=%d: antipodal emulation %.1e %.1e' % (tag, F, emu[0], emu[1]))
        assert ci.close(Ct, dCt, want, np.zeros((L, 2)), R, b2), (tag, 'antipodal bar 2', b2)
    for name, vecs, period in (('alternating', ci.alternating(N), 2), ('three_site', ci.three_site(N), 3)):
        Ct, dCt = run(ctx, form, opts, mode, vecs, R, F)
        want = ci.periodic_answer(L, period)
        eC, eD = ci.errors(Ct, dCt, want, np.zeros((L, 1)), R)
        print('[mobile] known answers %s F=%d: %s |dC| %.1e |d dC|(sqrt(R)-1) %.1e' % (tag, F, name, eC[0], eD[0]))
        assert ci.close(Ct, dCt, want, np.zeros((L, 1)), R, bar), (tag, name)
        if f32_transform:
            b2, emu = ci.bar2_of(vecs[:R * F].reshape(R, F, 1, 3), want, np.zeros((L, 1)), floor_columns=())
            print('[mobile] known answers %s F=%d: %s emulation %.1e' % (tag, F, name, emu[0]))
            assert ci.close(Ct, dCt, want, np.zeros((L, 1)), R, b2), (tag, name, 'bar 2', b2)


# ---- the pair kernels on the same inputs ---------------------------------------------------------------------------------------------------------
PAIRS = np.array([(i, i) for i in range(8)] + [(WALK_SLOW, JUMP), (WOBBLE, WHITE), (SCALED, ANTIPODAL)], dtype=np.int32)


def check_pairs(tag, F, got, ref, R, bar, Cp, dCp, bar_diag):
    P0, C, dC = got
    P0r, Cr, dCr = ref
    scale = ci.scale_of(np.vstack([Cr, P0r[None, :]]))
    eC, eD = ci.errors(C, dC, Cr, dCr, R)
    print('\n[mobile] %s F=%d R=%d  |dC|/scale per pair   %s' % (tag, F, R, ' '.join('%.1e' % e for e in eC)))
    print('[mobile] %s F=%d R=%d  |d dC|(sqrt(R)-1)/scale   %s   |dP0| %.1e' % (tag, F, R, ' '.join('%.1e' % e for e in eD),
                                                                               np.max(np.abs(P0 - P0r) / scale)))
    assert ci.close(C, dC, Cr, dCr, R, bar) and np.all(np.abs(P0 - P0r) <= bar * scale), tag
    # the diagonal pairs are kernel 1's C(t): two results that each lie within their bar of the definition
    assert ci.close(C[:, :8], dC[:, :8], Cp, dCp, R, bar_diag), tag


@pytest.mark.parametrize('F', [257, 1000])
def test_pair_kernel_direct(ctx, F):
    """k_ct_cross (every chunk it can stage and that is shorter than "ct_cross_long_min_frames" goes to it: ct._ct_cross), float32 dot
    products and float64 throughout"""
    vecs, R = ci.case_input(F)
    v4 = vecs[:R * F].reshape(R, F, 8, 3)
    assert F <= ctx.ct_cross_max_frames() and F < ctx.ct_cross_long_min_frames
    for mode, bar in ((0, ci.NORTH_STAR), (1, ci.BAR_F64)):
        Cp, dCp = run(ctx, formulation(ctx, {}, mode, F), {}, mode, vecs, R, F)
        for sym in (0, 1):
            with options(ctx):
                got = hostct.calculate_Ct_cross(v4, PAIRS, symmetric=bool(sym), ctx=ctx, mode=mode)
            check_pairs('k_ct_cross mode=%d sym=%d' % (mode, sym), F, got, oracle_cross(v4, PAIRS, sym), R, bar, Cp, dCp, bar)


def test_pair_kernel_blocked(ctx):
    """sr_ct_cross_long at its smallest length, 5462 ("ct_cross_long_min_frames" = 5462 hands it the chunks k_ct_cross could stage).
    That the blocked form ran: the dispatch's result is ResidentVectors.ct_cross_long's bit for bit and not ct_cross's.  Bars: 1e-6 on
    every pair; on the diagonal pairs also bar 2 of kernel 1's float32 transforms (the emulation is an autocorrelation)."""
    F = 5462
    vecs, R, Cr1, dCr1 = ci.case(F)
    v4 = vecs[:R * F].reshape(R, F, 8, 3)
    b2, _ = ci.bar2(F)
    Cp, dCp = run(ctx, BLOCKED, {'ct_long_min_frames': 5462}, 0, vecs, R, F)
    with options(ctx, ct_cross_long_min_frames=5462):
        with ctx.vectors(8, R * F) as rv:
            rv.append(np.ascontiguousarray(vecs[:R * F]))
            for sym in (0, 1):
                got = hostct.calculate_Ct_cross_resident(rv, PAIRS, R, F, symmetric=bool(sym))
                assert got[1].tobytes() == rv.ct_cross_long(R, F, PAIRS, sym=sym)[1].tobytes()
                assert got[1].tobytes() != rv.ct_cross(R, F, PAIRS, sym=sym)[1].tobytes()
                check_pairs('sr_ct_cross_long sym=%d' % sym, F, got, oracle_cross(v4, PAIRS, sym), R, ci.NORTH_STAR, Cp, dCp,
                            ci.NORTH_STAR)
                assert ci.close(got[1][:, :8], got[2][:, :8], Cr1, dCr1, R, b2), 'bar 2 on the diagonal pairs'
