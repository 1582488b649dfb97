"""
Inputs, the float64 reference, the comparison and a float32 emulation for the tests of the distance-weighted correlation functions
(csrc/sr_ct_dipolar.hip, sr_ct_dipolar_cross.hip, sr_ct_dipolar_long.hip) on MOBILE pairs whose distance varies by factors:
tests/test_ct_dipolar_inputs_host.py (the conditions on the inputs, no GPU) and tests/test_gpu_ct_dipolar_mobile.py.

make_pairs of tests/test_gpu_ct_dipolar.py wobbles 0.15 rad about a fixed axis at a distance r0 exp(y), sigma(y) = 0.1: w = (r_ref / r)^3
spans less than a factor of 3, C_dd stays above 0.4 and every chunk looks like every other.  Here the directions are the generators of
ct_inputs (wobble, walk, jump, white) and the distances are six processes (PROCESSES): w spans four orders of magnitude, contact
episodes put 64 frames of w ~ 1 into a chunk whose other frames have w ~ 0.016, one chunk holds a contact and the next none, and
C_dd passes through zero.  Everything is built from the integer hashing of spinrelax_amd.synth, vechist_inputs.gauss and IEEE-exact
float64 + - * / sqrt (the exponential too: _exp64), rounded once to float32, so the arrays are the same bit for bit wherever numpy
runs (sha256 of a 300-frame array of each: tests/test_ct_dipolar_inputs_host.py).

The comparison is ct_inputs.close: ABSOLUTE at scale_v = max(1, max_t |C_ref[:, v]|), no element excluded.
"""
import numpy as np
import scipy.fft as sfft

import ct_inputs as ci
from ct_inputs import EMU_FACTOR, NORTH_STAR, STEP_FAST, STEP_SLOW, P_JUMP, _once
from spinrelax_amd import synth
from spinrelax_amd.synth import _hash, _uniform
from test_ct_dipolar_long_host import oracle_dcross_fft, oracle_dipolar_fft
from test_gpu_ct_dipolar import oracle_dipolar, planes_of
from test_gpu_ct_dipolar_cross import oracle_dcross
from vechist_inputs import gauss

MILD, WIDE, CONTACT, ANGLE, SPIKE, CONST = range(6)
PROCESSES = ('mild', 'wide', 'contact', 'angle', 'spike', 'const')
# the series of mixed(): direction x distance process
WOB_MILD, SLOW_WIDE, FAST_WIDE, JUMP_CONTACT, WHITE_CONTACT, SLOW_ANGLE, FAST_SPIKE, SLOW_CONST, SHARED_CONTACT = range(9)
SERIES = ('wobble*mild', 'walk.02*wide', 'walk.15*wide', 'jump*contact', 'white*contact', 'walk.02*angle', 'walk.15*spike',
          'walk.02*const', 'shared*contact')
NSER = len(SERIES)
WIDE_SERIES = (SLOW_WIDE, FAST_WIDE)
CONTACT_SERIES = (JUMP_CONTACT, WHITE_CONTACT, SHARED_CONTACT)
MOBILE_SERIES = (FAST_WIDE, JUMP_CONTACT, WHITE_CONTACT, FAST_SPIKE)     # walk.15, jump and white directions
# the cross form: (i, i) of a WIDE and a CONTACT series; (i, j) and (j, i) of two series of different mobility; two independent series
# (P0 and C near zero at every lag); the shared direction (series 8 repeats the direction of series 1 under an independent CONTACT
# distance); one repeated pair
PAIRS = np.array([(SLOW_WIDE, SLOW_WIDE), (JUMP_CONTACT, JUMP_CONTACT), (SLOW_WIDE, FAST_WIDE), (FAST_WIDE, SLOW_WIDE),
                  (JUMP_CONTACT, WHITE_CONTACT), (SLOW_WIDE, SHARED_CONTACT), (SLOW_WIDE, FAST_WIDE)], dtype=np.int32)
PAIR_NAMES = ('wide,wide(i,i)', 'contact(i,i)', 'slow,fast', 'fast,slow', 'independent', 'shared', 'slow,fast again')
P_II_WIDE, P_II_CONTACT, P_IJ, P_JI, P_INDEP, P_SHARED, P_REPEAT = range(7)

R_NEAR, R_FAR, R_SPIKE, R_CONST = 0.25, 1.0, 0.05, np.float32(0.37)
NEAR_BELOW = 0.5              # a frame of a CONTACT series is "near" when r < 0.5 (near 0.25, far 1, 5 % jitter each)
EPISODE = 30                  # mean length of a contact episode, frames
MOBILE_FROM = ci.MOBILE_FROM  # the mobility conditions hold from this chunk length on
CONTACT_FROM = 1000           # ... the contact conditions (a chunk without a near frame, an episode of >= 64 frames) from this one
TAIL = 16                     # trailing frames: room for the chunk starts [0, F + 4, 2 F + 11] of the odd-start case


def _exp64(y):
    """exp(y) for |y| < 8 from + * / alone (np.exp may differ in the last bit between builds of numpy): the Taylor polynomial of degree
    12 at y / 1024, squared ten times; relative error about 1e-13"""
    z = np.asarray(y, dtype=np.float64) / 1024.0
    s = np.ones_like(z)
    for n in range(12, 0, -1):
        s = 1.0 + s * z / float(n)
    for _ in range(10):
        s = s * s
    return s


def _ar1(N, V, seed, sigma, rho):
    """stationary AR(1) (N, V) of standard deviation sigma: make_pairs' recursion on gauss()"""
    g = gauss((N + 1, V), seed)
    y = np.empty((N, V))
    x = sigma * g[0]
    k = sigma * np.sqrt(1.0 - rho * rho)
    for t in range(N):
        x = rho * x + k * g[t + 1]
        y[t] = x
    return y


def _r0(V, seed):
    """base distances 0.18 .. 0.48, make_pairs' range"""
    return 0.18 + 0.30 * _uniform(np.arange(V, dtype=np.uint64), seed * 1000 + 51)


# ---- the distance processes: float64 (N, V) ---------------------------------------------------------------------------------------------
def _mild64(N, V, seed):
    return _r0(V, seed)[None] * _exp64(_ar1(N, V, seed * 10 + 1, 0.1, 0.9))


def _wide64(N, V, seed):
    return _r0(V, seed + 1)[None] * _exp64(_ar1(N, V, seed * 10 + 2, 0.5, 0.99))


def _near_mask(N, V, seed, F):
    """two-state Markov chain: far -> near with probability 1 / F per frame, near -> far with 1 / EPISODE; starts far"""
    n = np.arange(N, dtype=np.uint64)[:, None] * np.uint64(V) + np.arange(V, dtype=np.uint64)[None, :]
    u = _uniform(n, seed * 1000 + 61)
    near = np.zeros((N, V), dtype=bool)
    state = np.zeros(V, dtype=bool)
    p_in, p_out = 1.0 / F, 1.0 / EPISODE
    for t in range(N):
        state = np.where(state, u[t] >= p_out, u[t] < p_in)
        near[t] = state
    return near


def _contact64(N, V, seed, F):
    jitter = _exp64(0.05 * gauss((N, V), seed * 10 + 3))
    return np.where(_near_mask(N, V, seed, F), R_NEAR, R_FAR) * jitter


def _angle64(uz, seed):
    """r = r0 (1 + 0.6 u_z) of the directions' z components uz (N, V): the distance tied to the orientation"""
    return _r0(uz.shape[1], seed + 2)[None] * (1.0 + 0.6 * np.asarray(uz, dtype=np.float64))


def spike_frame(N, seed):
    return int(_hash(np.array([0], dtype=np.uint64), seed * 1000 + 71)[0] % np.uint64(N))


def _spike64(N, V, seed):
    r = R_FAR * _exp64(0.05 * gauss((N, V), seed * 10 + 4))
    r[spike_frame(N, seed)] = R_SPIKE
    return r


def process(kind, N, V, seed, F=100):
    """(N, V) float32 distances of one process, read-only, cached (ANGLE: of the directions ct_inputs.walk(N, V, seed, 0.02))"""
    def make():
        if kind == MILD:
            r = _mild64(N, V, seed)
        elif kind == WIDE:
            r = _wide64(N, V, seed)
        elif kind == CONTACT:
            r = _contact64(N, V, seed, F)
        elif kind == ANGLE:
            r = _angle64(ci.walk(N, V, seed, STEP_SLOW)[..., 2], seed)
        elif kind == SPIKE:
            r = _spike64(N, V, seed)
        else:
            r = np.full((N, V), R_CONST, dtype=np.float64)
        return r.astype(np.float32)
    return _once(('dip_process', kind, N, V, seed, F), make)


# ---- the mixed input --------------------------------------------------------------------------------------------------------------------
def mixed(N, seed, F):
    """(u (N, 9, 3) unit vectors, dist (N, 9), raw = float32(u dist)) float32, read-only: one launch of the nine SERIES.  F sets the entry
    probability of the CONTACT chain: about one episode per chunk of F frames"""
    def make():
        u = np.empty((N, NSER, 3), dtype=np.float32)
        d = np.empty((N, NSER), dtype=np.float32)
        w = ci.walk(N, 5, seed, (STEP_SLOW, STEP_FAST, STEP_SLOW, STEP_FAST, STEP_SLOW))
        u[:, WOB_MILD] = synth.synth_vectors(N, 1, seed)[:, 0]
        u[:, SLOW_WIDE], u[:, FAST_WIDE], u[:, SLOW_ANGLE], u[:, FAST_SPIKE], u[:, SLOW_CONST] = (w[:, k] for k in range(5))
        u[:, JUMP_CONTACT] = ci.jump(N, 1, seed, P_JUMP)[:, 0]
        u[:, WHITE_CONTACT] = ci.white(N, 1, seed + 1)[:, 0]
        u[:, SHARED_CONTACT] = u[:, SLOW_WIDE]
        d[:, WOB_MILD] = _mild64(N, 1, seed)[:, 0]
        d[:, [SLOW_WIDE, FAST_WIDE]] = _wide64(N, 2, seed)
        d[:, [JUMP_CONTACT, WHITE_CONTACT, SHARED_CONTACT]] = _contact64(N, 3, seed, F)
        d[:, SLOW_ANGLE] = _angle64(u[:, SLOW_ANGLE, 2:3], seed)[:, 0]
        d[:, FAST_SPIKE] = _spike64(N, 1, seed)[:, 0]
        d[:, SLOW_CONST] = R_CONST
        raw = (u.astype(np.float64) * d.astype(np.float64)[..., None]).astype(np.float32)
        for a in (u, d, raw):
            a.setflags(write=False)
        return u, d, raw
    return _once(('dip_mixed', N, seed, F), make)


# ---- the lengths of tests/test_gpu_ct_dipolar_mobile.py: chunk length F -> seed of mixed(); R = 3 throughout -------------------------------
# The seeds were chosen by scanning 1, 2, ... for the first that meets the conditions of tests/test_ct_dipolar_inputs_host.py at that
# length (at 10017 for both chunk tables, the regular one and ODD_STARTS).
R = 3
CASES = {128: 361, 257: 64, 1000: 4, 4097: 1, 4100: 1, 4897: 2, 5462: 2, 8193: 1, 10017: 2, 12289: 1}
LAG_BY_LAG_UPTO = 4100        # the lag-by-lag oracles of the direct kernels' tests up to here, their FFT forms beyond


def odd_starts(F):
    """chunk starts 0, F + 4 (odd for odd F) and 2 F + 11"""
    return np.array([0, F + 4, 2 * F + 11], dtype=np.int64)


def case_input(F):
    """(u, dist, raw) of one length, R F + TAIL frames"""
    return mixed(R * F + TAIL, CASES[F], F)


def chunked(x, F, starts=None):
    starts = np.arange(R) * F if starts is None else starts
    return np.stack([x[s:s + F] for s in starts])


def planes(F, form='raw', held=None):
    """float64 a (N, 9, 3), w (N, 9), r_ref (9) of the first `held` frames (default R F: what calculate_Ct_dipolar holds) of one
    input form, 'raw' or 'dist'"""
    u, d, raw = case_input(F)
    n = R * F if held is None else held
    return planes_of(raw[:n], None) if form == 'raw' else planes_of(u[:n], d[:n])


# ---- the float64 reference -----------------------------------------------------------------------------------------------------------------
def reference_auto(F, form='raw', starts=None):
    """(C, dC, reff6, reff3, S2rad) of the definition in float64, computed once.  starts: the chunk table; then r_ref runs over all
    R F + TAIL frames (resident vectors), else over the R F frames of the regular chunks"""
    def make():
        u, d, raw = case_input(F)
        n = R * F if starts is None else R * F + TAIL
        vec, dist = (raw[:n], None) if form == 'raw' else (u[:n], d[:n])
        if F <= LAG_BY_LAG_UPTO:
            return oracle_dipolar(vec, dist, R, F, starts)
        return oracle_dipolar_fft(vec, dist, R, F, starts)
    return _once(('dip_ref_auto', F, form, None if starts is None else tuple(starts)), make)


def reference_pairs(F, sym, form='raw'):
    """(P0, dP0, C, dC, reff6) of PAIRS, computed once"""
    def make():
        u, d, raw = case_input(F)
        n = R * F
        vec, dist = (raw[:n], None) if form == 'raw' else (u[:n], d[:n])
        if F <= LAG_BY_LAG_UPTO:
            return oracle_dcross(vec, dist, PAIRS, sym, R, F)
        return oracle_dcross_fft(vec, dist, PAIRS, sym, R, F)
    return _once(('dip_ref_pairs', F, sym, form), make)


# ---- the comparison ------------------------------------------------------------------------------------------------------------------------
def close_p0(P0, dP0, P0r, dP0r, bar):
    """ct_inputs.close on the equal-time values as one row of lags: absolute at max(1, |P0_ref|), the dC rule for dP0"""
    return ci.close(np.asarray(P0)[None], np.asarray(dP0)[None], np.asarray(P0r)[None], np.asarray(dP0r)[None], R, bar)


def errors_p0(P0, dP0, P0r, dP0r):
    return ci.errors(np.asarray(P0)[None], np.asarray(dP0)[None], np.asarray(P0r)[None], np.asarray(dP0r)[None], R)


# ---- the blocked arithmetic in numpy -----------------------------------------------------------------------------------------------------
_SIGNALS = (lambda x, y, z: (2 * z * z - x * x - y * y, 1.0 / 6.0), lambda x, y, z: (x * x - y * y, 0.5), lambda x, y, z: (x * y, 2.0),
            lambda x, y, z: (x * z, 2.0), lambda x, y, z: (y * z, 2.0))


def emulate_dipolar_f32(a4, M, w4=None, restore=(True,) * 5):
    """C_dd, dC_dd (L, V) of the planes a4 (R, F, V, 3) (w4 (R, F, V): the w plane; None: |a|^2) by the five-signal algebra of the
    sr_ct_dipolar_long.hip header with scipy's float32 transforms of M points: the five traceless components of a (x) a, the float32
    chunk mean of each removed before the signal is rounded to float32, one float32 power spectrum and one inverse transform, what
    the means removed restored in float64; no |a|^2 signal, no eps term; normalised by the float64 chunk means of w^2.  restore[c]
    False: the mean of signal c is NOT restored (the host tests show that this breaks it).  Shares no code with the kernels."""
    a4 = np.asarray(a4, dtype=np.float32)
    R_, F, V, _ = a4.shape
    L = F // 2
    assert M >= F + L
    x, y, z = (a4[..., k].astype(np.float64) for k in range(3))
    w = x * x + y * y + z * z if w4 is None else np.asarray(w4, dtype=np.float64)
    lag = np.arange(L + 1)
    nlag = (F - lag)[None, :, None]
    P = np.zeros((R_, M // 2 + 1, V), dtype=np.float32)
    e = np.zeros((R_, F, V))
    const = np.zeros((R_, L + 1, V))
    for c, sig in enumerate(_SIGNALS):
        q, wt = sig(x, y, z)
        m = q.mean(axis=1, keepdims=True).astype(np.float32).astype(np.float64)
        d = (q - m).astype(np.float32)
        D = sfft.rfft(d, n=M, axis=1)
        assert D.dtype == np.complex64
        P += np.float32(wt) * (D.real * D.real + D.imag * D.imag)
        if restore[c]:
            e = e + wt * m * d.astype(np.float64)
            const = const + wt * (m * m) * nlag
    s = sfft.irfft(P, n=M, axis=1)
    assert s.dtype == np.float32 and P.dtype == np.float32
    PE = np.concatenate([np.zeros((R_, 1, V)), np.cumsum(e, axis=1)], axis=1)
    S = s[:, :L + 1].astype(np.float64) + PE[:, F - lag] + (PE[:, F:F + 1] - PE[:, lag]) + const
    c_r = 1.5 * S[:, 1:] / nlag[:, 1:]                                    # (R, L, V)
    n = ((w * w).sum(axis=1) / F).mean(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        return c_r.mean(axis=0) / n, c_r.std(axis=0) / (np.sqrt(R_) - 1.0) / n


def f32_planes(a, w):
    """what the pack writes: the float64 planes rounded once to float32"""
    return a.astype(np.float32), w.astype(np.float32)


def bar2_of(a4, w4, Cr, dCr):
    """bar 2 of the blocked forms, per series: EMU_FACTOR x max_t |emulate_dipolar_f32 - oracle| / scale on these very chunks, never
    more than the north star.  No series of mixed() has constant products, so no series takes ct_inputs.EMU_FLOOR.  Returns (bar per
    series, the emulation's error per series)."""
    Ce, dCe = emulate_dipolar_f32(a4, ci.transform_points(a4.shape[1]), w4)
    emu, _ = ci.errors(Ce, dCe, Cr, dCr, a4.shape[0])
    return np.minimum(NORTH_STAR, EMU_FACTOR * emu), emu


def bar2(F, starts=None):
    """bar2_of the chunks of case_input(F) in the raw form, computed once"""
    def make():
        a, w, _ = planes(F, 'raw', None if starts is None else R * F + TAIL)
        a32, w32 = f32_planes(a, w)
        ref = reference_auto(F, 'raw', starts)
        return bar2_of(chunked(a32, F, starts), chunked(w32, F, starts), ref[0], ref[1])
    return _once(('dip_bar2', F, None if starts is None else tuple(starts)), make)


# ---- the conditions that keep the inputs hard: figures of one (length, seed), and which of them fail ----------------------------------------
def _longest_run(mask):
    best = run = 0
    for m in mask:
        run = run + 1 if m else 0
        best = max(best, run)
    return best


def figures(F, seed, starts=None):
    """what tests/test_ct_dipolar_inputs_host.py asserts about mixed(R F + TAIL, seed, F) on the chunks at `starts` (default r F), as a
    dict; the per-chunk C_dd by the FFT oracle (held to 1e-12 of the lag-by-lag one)"""
    from test_ct_dipolar_long_host import fft_core, fft_cross_core
    u, d, raw = mixed(R * F + TAIL, seed, F)
    n = R * F if starts is None else R * F + TAIL
    a, w, _ = planes_of(raw[:n], None)
    a4, w4 = chunked(a, F, starts), chunked(w, F, starts)
    st = np.arange(R) * F if starts is None else np.asarray(starts)
    f = {}
    f['wide_min_w'] = w[:, list(WIDE_SERIES)].min(axis=0)
    m2 = (w4[:, :, list(WIDE_SERIES)] ** 2).mean(axis=1)                       # (R, 2)
    f['wide_chunk_ratio'] = float(np.max(m2.max(axis=0) / m2.min(axis=0)))
    near = chunked(d[:n, list(CONTACT_SERIES)] < NEAR_BELOW, F, starts)         # (R, F, 3)
    f['contact_chunks_without'] = int(np.count_nonzero(~near.any(axis=1)))
    f['contact_longest_episode'] = max(_longest_run(near[r, :, k]) for r in range(R) for k in range(near.shape[2]))
    ws = w[:, FAST_SPIKE]
    f['spike_frames_w1'] = int(np.count_nonzero(ws == 1.0))
    f['spike_other_max_w'] = float(np.max(ws[ws != 1.0]))
    sf = spike_frame(R * F + TAIL, seed)
    f['spike_in_chunk'] = bool(np.any((st <= sf) & (sf < st + F)))
    f['angle_corr'] = float(np.corrcoef(d[:n, SLOW_ANGLE].astype(np.float64), u[:n, SLOW_ANGLE, 2].astype(np.float64))[0, 1])
    sign, small = [], []
    for r in range(R):
        C = fft_core(a4[r:r + 1], w4[r:r + 1])[0][:, list(MOBILE_SERIES)]
        sign.append((C.min(axis=0) < 0.0) & (C.max(axis=0) > 0.0))
        small.append(np.min(np.abs(C), axis=0))
    f['mobile_sign_change'] = np.array(sign)                                   # (R, 4)
    f['mobile_min_abs_C'] = np.array(small)
    f['wide_max_dC'] = fft_core(a4, w4)[1][:, list(WIDE_SERIES)].max(axis=0)
    f['P0'] = fft_cross_core(a4, w4, PAIRS, 1)[0]
    return f


def failed(f, F):
    """names of the conditions that the figures f of a chunk length F miss"""
    bad = []
    if not np.all(f['wide_min_w'] < 1e-3):
        bad.append('WIDE: min w < 1e-3 in every series')
    if not f['wide_chunk_ratio'] >= 4.0:
        bad.append('WIDE: chunk means of w^2 differ by a factor >= 4')
    if not (f['spike_frames_w1'] == 1 and f['spike_other_max_w'] < 1e-3 and f['spike_in_chunk']):
        bad.append('SPIKE: exactly one frame with w = 1, inside a chunk, every other w < 1e-3')
    if not f['angle_corr'] > 0.9:
        bad.append('ANGLE: corr(r, u_z) > 0.9')
    if F >= CONTACT_FROM:
        if not f['contact_chunks_without'] >= 1:
            bad.append('CONTACT: a (chunk, series) without a near frame')
        if not f['contact_longest_episode'] >= 64:
            bad.append('CONTACT: an episode of >= 64 near frames')
    if F >= MOBILE_FROM:
        if not np.all(f['mobile_sign_change']):
            bad.append('mobility: a sign change of C_dd in every chunk')
        if not np.all(f['mobile_min_abs_C'] < 1e-3):
            bad.append('mobility: a value of |C_dd| below 1e-3 in every chunk')
        if not np.max(f['wide_max_dC']) > 0.1:
            bad.append('mobility: max dC of a WIDE series > 0.1')
        if not (np.min(np.abs(f['P0'])) < 0.05 and np.max(f['P0']) > 0.5):
            bad.append('pairs: one |P0| < 0.05 and one P0 > 0.5')
    return bad
