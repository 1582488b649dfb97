"""
Inputs, the float64 reference and the comparison for the tests of kernel 1 (C(t), csrc/sr_ct*.hip) and of the pair kernels on MOBILE
vectors: tests/test_ct_inputs_host.py (the conditions on the inputs, no GPU) and tests/test_gpu_ct_mobile.py.

synth.synth_vectors (and make_vectors of the cross tests) wobble ~0.1 rad about a fixed mean: S2 is 0.9, C(t) stays between 0.68 and 1
and every product of two components is a large constant plus a small fluctuation -- the regime the float32-transform kernels
(k_ct_rfft32, k_ctl_*, sr_ct_cross_long) were designed around and measured in.  The generators here tumble (walk), jump between random
directions (jump) or are uncorrelated (white): C(t) decays to zero, changes sign, and differs strongly from chunk to chunk.  They use
the integer hashing of spinrelax_amd.synth and IEEE-exact float64 + - * / sqrt only, so the float32 arrays are the same bit for bit
wherever numpy runs (sha256 of a small array of each: tests/test_ct_inputs_host.py).

Where C(t) passes through zero a bar relative to the element says nothing, so close() is ABSOLUTE at the scale of C(0): per series
(column) scale_v = max(1, max_t |C_ref[:, v]|), and no element is ever excluded.

conftest.dct_close_f32_transform asserts 5e-8 absolute on the replicate means of the float32 transforms: that is the figure for the
ORDERED vectors of synth_vectors.  On the inputs of this module the float32 transforms are off by up to 2e-7 (emulate_f32 below and
the measured figures of docs/EXPERIMENTS.md section 27), which is why the tests of this module carry their own bars.
"""
import ctypes
import os
import subprocess

import numpy as np
import scipy.fft as sfft

from conftest import ROOT
from spinrelax_amd import synth
from spinrelax_amd.synth import _hash, _uniform
from vechist_inputs import gauss, iso

NORTH_STAR = 1e-6            # BASELINE.json: C(t) within 1e-6; the bar of the direct float32 kernel and bar 1 of the float32 transforms
BAR_F64 = 1e-12              # the float64 formulations (mode 1, k_ct_fft, k_ct_rfft)
BAR_EXACT = 4e-15            # constant products: the bar of the constant-vector tests of tests/test_gpu_parity.py
EMU_FACTOR = 4.0             # bar 2 of the float32 transforms: this many times the error of emulate_f32 on the same chunks
EMU_FLOOR = 2.0 ** -24       # ... of the ANTIPODAL series alone, where the emulation is exact: one float32 rounding of C(0) = 1 (bar2_of)
UNIT_TOL = 5e-7              # kUnitTolF of the kernels: | |u|^2 - 1 | below it at every frame -> five transforms

WOBBLE, WALK_SLOW, WALK_FAST, JUMP, WHITE, SCALED, ZEROS, ANTIPODAL = range(8)
KINDS = ('wobble', 'walk.02', 'walk.15', 'jump', 'white', 'scaled', 'zeros', 'antipodal')
UNIT_KINDS = (WOBBLE, WALK_SLOW, WALK_FAST, JUMP, WHITE, ANTIPODAL)
STEP_SLOW, STEP_FAST, P_JUMP = 0.02, 0.15, 0.01

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
        if isinstance(_cache[key], np.ndarray):
            _cache[key].setflags(write=False)
    return _cache[key]


def _unit64(g):
    return g / np.sqrt((g * g).sum(axis=-1))[..., None]


# ---- generators: float32 (N, V, 3), read-only, cached per key ---------------------------------------------------------------------------
def _walk64(N, V, seed, step):
    """step: a number or one per vector"""
    g = gauss((N, V, 3), seed) * (np.ones(V) * np.asarray(step, dtype=np.float64))[None, :, None]
    out = np.empty((N, V, 3))
    u = _unit64(gauss((V, 3), seed + 7919))
    for n in range(N):
        out[n] = u
        u = u + g[n]
        u = u / np.sqrt((u * u).sum(axis=-1))[:, None]
    return out


def walk(N, V, seed, step):
    """isotropic rotational diffusion: u_{n+1} = normalise(u_n + step g_n) in float64, g standard normal per component, the start
    uniform on the sphere.  step 0.02: C(t) decays over ~800 frames and differs strongly from chunk to chunk; step 0.15: it decays
    within ~15 frames and is noise around zero, with sign changes, after that."""
    return _once(('walk', N, V, seed, step), lambda: _walk64(N, V, seed, step).astype(np.float32))


def jump(N, V, seed, p):
    """piecewise constant: with probability p per frame the vector jumps to a new direction uniform on the sphere"""
    def make():
        dirs = iso(N, V, seed)
        n = np.arange(N, dtype=np.uint64)[:, None] * np.uint64(V) + np.arange(V, dtype=np.uint64)[None, :]
        flag = _uniform(n, seed * 1000 + 31) < p
        last = np.maximum.accumulate(np.where(flag, np.arange(N)[:, None], 0), axis=0)         # frame of the latest jump (frame 0 at the start)
        return np.take_along_axis(dirs, last[:, :, None], axis=0)
    return _once(('jump', N, V, seed, p), make)


def white(N, V, seed):
    """uncorrelated directions uniform on the sphere (vechist_inputs.iso): C(t) is ~0 at every lag >= 1"""
    return _once(('white', N, V, seed), lambda: iso(N, V, seed))


def _signs(N, seed):
    return np.where((_hash(np.arange(N, dtype=np.uint64), seed * 1000 + 41) >> np.uint64(63)) == 0, 1.0, -1.0).astype(np.float32)


def antipodal(N, seed):
    """u_n = (-1)^h(n) u_0 with hashed signs, two series: u_0 = z, and u_0 a float32-rounded direction that lies on no axis.  Every
    product of two components is constant: C(t) = 1.5 |u_0|^4 - 0.5 at every lag and dC(t) = 0 (antipodal_answer)."""
    def make():
        u0 = np.stack([np.array([0.0, 0.0, 1.0], dtype=np.float32), iso(1, 1, seed)[0, 0]])
        return _signs(N, seed)[:, None, None] * u0[None]
    return _once(('antipodal', N, seed), make)


def antipodal_answer(vecs):
    """C(t) of every series of antipodal(): 1.5 |u_0|^4 - 0.5 from the float32 components in float64 (1 exactly for u_0 = z)"""
    s = (np.asarray(vecs[0], dtype=np.float64) ** 2).sum(axis=-1)
    return 1.5 * s * s - 0.5


_AXES = np.eye(3, dtype=np.float32)


def alternating(N):
    """x for even n, y for odd n: C(odd) = -0.5, the lower bound of P2, and C(even) = 1"""
    return _once(('alternating', N), lambda: _AXES[np.arange(N) % 2][:, None, :].copy())


def three_site(N):
    """x, y, z, x, y, z, ...: C(k) = 1 for k a multiple of 3, otherwise -0.5"""
    return _once(('three_site', N), lambda: _AXES[np.arange(N) % 3][:, None, :].copy())


def periodic_answer(L, period):
    """C(t) at the lags 1 .. L of alternating (period 2) and three_site (period 3), (L, 1)"""
    return np.where(np.arange(1, L + 1) % period == 0, 1.0, -0.5)[:, None]


def zero_frames(N):
    """the frames of mixed()'s series ZEROS that hold zero vectors: 40 of them from frame 100 (fewer and earlier in a short input)"""
    start = min(100, N // 3)
    return start, min(N, start + min(40, max(1, N // 16)))


def mixed(N, seed):
    """one launch of 8 series, one of each kind (KINDS): the choice between five and six transforms per series and the means per
    (chunk, signal) side by side in one grid"""
    def make():
        v = np.empty((N, 8, 3), dtype=np.float32)
        v[:, WOBBLE] = synth.synth_vectors(N, 1, seed)[:, 0]
        w = _walk64(N, 3, seed, (STEP_SLOW, STEP_FAST, STEP_SLOW)).astype(np.float32)
        v[:, WALK_SLOW], v[:, WALK_FAST] = w[:, 0], w[:, 1]
        j = jump(N, 2, seed, P_JUMP)
        v[:, JUMP] = j[:, 0]
        v[:, WHITE] = iso(N, 1, seed + 1)[:, 0]
        v[:, SCALED] = w[:, 2] * np.float32(1.7)               # not unit: the sixth signal |u|^2
        v[:, ZEROS] = j[:, 1]
        z0, z1 = zero_frames(N)
        v[z0:z1, ZEROS] = 0.0                                  # the 0/0 guard of vecnorm_NDarray
        v[:, ANTIPODAL] = antipodal(N, seed)[:, 1]
        return v
    return _once(('mixed', N, seed), make)


# ---- the lengths of tests/test_gpu_ct_mobile.py: chunk length F -> (R, seed of mixed()) ---------------------------------------------------
# The seeds were chosen by scanning 1, 2, ... for the first that meets the conditions of tests/test_ct_inputs_host.py at that length.
TAIL = 3                      # trailing frames that every kernel must ignore
CASES = {
    7: (3, 1), 255: (3, 43), 257: (3, 43), 682: (3, 19), 683: (3, 15), 1000: (3, 2),
    684: (3, 37), 1365: (3, 3), 1366: (3, 3), 2730: (3, 1), 2731: (3, 1),
    3001: (3, 1), 4095: (3, 1), 4096: (3, 1), 4097: (3, 1), 5461: (3, 1),
    5462: (3, 1), 8193: (3, 1), 12289: (2, 1), 16384: (2, 1),
}
MOBILE_FROM = 682             # from this length on every chunk of walk.15, jump and white has a zero crossing AND a value below 1e-3, and
                              # the slow walk max dC(t) > 0.02 (255, 257: no seed of 1 .. 1499 gives the value below 1e-3 in all nine
                              # (chunk, series) at L = 127, the zero crossing alone holds; 7 has three lags)
CHUNK_START_SEEDS = (1, 101)  # the two "files" of chunk_start_case


def case_input(F):
    """(vecs (R F + TAIL, 8, 3), R) of one length"""
    R, seed = CASES[F]
    return mixed(R * F + TAIL, seed), R


def chunk_start_case(F):
    """two "files" of mixed(), 2 F + 1 and F + 9 frames: (cat, starts, R = 3, v4 (R, F, 8, 3), Cr, dCr).  The first file's odd tail
    stays in cat, so the third chunk starts at an odd frame"""
    def make():
        a, b = mixed(2 * F + 1, CHUNK_START_SEEDS[0]), mixed(F + 9, CHUNK_START_SEEDS[1])
        cat = np.ascontiguousarray(np.concatenate([a, b]))
        starts = np.array([0, F, 2 * F + 1], dtype=np.int64)
        v4 = np.stack([cat[st:st + F] for st in starts])
        v4.setflags(write=False)
        cat.setflags(write=False)
        return (cat, starts, 3, v4) + reference(v4)
    return _once(('chunk_start_case', F), make)


def case(F):
    """(vecs, R, Cr, dCr) of one length: the input and its oracle, computed once"""
    def make():
        vecs, R = case_input(F)
        return (vecs, R) + reference(vecs[:R * F].reshape(R, F, 8, 3))
    return _once(('case', F), make)


# ---- the float64 reference -----------------------------------------------------------------------------------------------------------
def liboracle():
    def load():
        so = os.path.join(ROOT, 'oracle', 'libsr_oracle.so')
        if not os.path.isfile(so):
            subprocess.check_call(['make', '-C', os.path.join(ROOT, 'oracle'), 'libsr_oracle.so'])
        lib = ctypes.CDLL(so)
        lib.sr_oracle_ct_palmer_f64.restype = ctypes.c_int
        return lib
    return _once('liboracle', load)


def c_oracle_ct(lib, v4):
    """the plain-C float64 restatement of calculate_Ct_Palmer (oracle/ct_palmer_oracle.c): v4 (R, F, V, 3) -> Ct, dCt (F // 2, V)"""
    v4 = np.ascontiguousarray(v4, dtype=np.float32)
    R, F, V, _ = v4.shape
    L = F // 2
    Ct = np.empty((L, V))
    dCt = np.empty((L, V))
    rc = lib.sr_oracle_ct_palmer_f64(v4.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(R), ctypes.c_int64(F),
                                     ctypes.c_int64(V), Ct.ctypes.data_as(ctypes.c_void_p),
                                     dCt.ctypes.data_as(ctypes.c_void_p), None)
    assert rc == 0
    return Ct, dCt


def reference(v4):
    return c_oracle_ct(liboracle(), v4)


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
def scale_of(Cr):
    return np.maximum(1.0, np.max(np.abs(Cr), axis=0))


def errors(Ct, dCt, Cr, dCr, R):
    """per series: max_t |Ct - Cr| / scale and max_t |dCt - dCr| (sqrt(R) - 1) / scale -- the error of C(t) and the error of the
    replicate means that the one of dC(t) stands for (R = 1: 0 where both are NaN, inf otherwise)"""
    scale = scale_of(Cr)
    eC = np.max(np.abs(Ct - Cr), axis=0) / scale
    if R == 1:
        eD = np.where(np.all(np.isnan(dCt) & np.isnan(dCr), axis=0), 0.0, np.inf)
    else:
        eD = np.max(np.abs(dCt - dCr), axis=0) * (np.sqrt(R) - 1.0) / scale
    return eC, eD


def close(Ct, dCt, Cr, dCr, R, bar):
    """|Ct - Cr| <= bar scale_v at every lag, scale_v = max(1, max_t |Cr[:, v]|), and |dCt - dCr| <= max(1e-6 |dCr|, bar scale_v /
    (sqrt(R) - 1)), the propagation through the standard deviation that dct_close of tests/test_gpu_parity.py documents.  bar: one
    number or one per series.  No element is excluded; R = 1: dC(t) is NaN on both sides.  NaN anywhere else fails."""
    Ct, dCt, Cr, dCr = (np.asarray(a, dtype=np.float64) for a in (Ct, dCt, Cr, dCr))
    if not (Ct.shape == dCt.shape == Cr.shape == dCr.shape):
        return False
    lim = (np.ones(Cr.shape[1]) * np.asarray(bar, dtype=np.float64) * scale_of(Cr))[None, :]
    if not np.all(np.abs(Ct - Cr) <= lim):
        return False
    if R == 1:
        return bool(np.all(np.isnan(dCt)) and np.all(np.isnan(dCr)))
    return bool(np.all(np.abs(dCt - dCr) <= np.maximum(1e-6 * np.abs(dCr), lim / (np.sqrt(R) - 1.0))))


# ---- the float32-transform arithmetic in numpy -------------------------------------------------------------------------------------------
def emulate_f32(v4, M):
    """C(t), dC(t) (L, V) of v4 (R, F, V, 3) by the decomposition of the sr_ct32.hip header with scipy's float32 transforms of M points
    (pocketfft): the five traceless components (and |u|^2 for a (chunk, series) with a frame outside the unit tolerance), the float32
    chunk mean of each removed before the signal is rounded to float32, one float32 power spectrum and one inverse transform, what
    the means removed restored in float64.  An implementation of the same algebra that shares no code with the kernels."""
    v4 = np.asarray(v4, dtype=np.float32)
    R, F, V, _ = v4.shape
    L = F // 2
    assert M >= F + L
    x, y, z = (v4[..., k].astype(np.float64) for k in range(3))            # (R, F, V)
    n2 = x * x + y * y + z * z
    eps = n2 - 1.0
    unit = (np.max(np.abs(eps), axis=1, keepdims=True) < UNIT_TOL)         # (R, 1, V)
    lag = np.arange(L + 1)
    nlag = (F - lag)[None, :, None]
    sigs = [(2 * z * z - x * x - y * y, 1.0 / 6.0), (x * x - y * y, 0.5), (x * y, 2.0), (x * z, 2.0), (y * z, 2.0),
            (n2, np.where(unit, 0.0, 1.0 / 3.0))]
    e = np.where(unit, eps / 3.0, 0.0)
    const = np.where(unit, 1.0 / 3.0, 0.0) * nlag
    P = np.zeros((R, M // 2 + 1, V), dtype=np.float32)
    for a, w in sigs:
        m = a.mean(axis=1, keepdims=True).astype(np.float32).astype(np.float64)
        d = (a - m).astype(np.float32)                                      # one rounding, like the kernel's fma
        D = sfft.rfft(d, n=M, axis=1)
        assert D.dtype == np.complex64
        P += np.asarray(w, dtype=np.float32) * (D.real * D.real + D.imag * D.imag)
        e = e + w * m * d.astype(np.float64)
        const = const + w * (m * m) * nlag
    s = sfft.irfft(P, n=M, axis=1)
    assert s.dtype == np.float32 and P.dtype == np.float32
    PE = np.concatenate([np.zeros((R, 1, V)), np.cumsum(e, axis=1)], axis=1)
    S = s[:, :L + 1].astype(np.float64) + PE[:, F - lag] + (PE[:, F:F + 1] - PE[:, lag]) + const
    p = 1.5 * (S[:, 1:] / nlag[:, 1:]) - 0.5                                # (R, L, V)
    with np.errstate(divide='ignore', invalid='ignore'):
        return p.mean(axis=0), p.std(axis=0) / (np.sqrt(R) - 1.0)


def transform_points(F):
    """points of the one transform that holds a chunk and its L lags: 2048, 4096, 6144 or 8192 as k_ct_rfft32 chooses them; for the
    blocked kernels' lengths the next power of two (one transform of the whole chunk, not 8192 points per block: the blocked
    form's rounding is that of its block transforms, and a per-block emulation would be a second implementation of the index
    algebra that tests/test_ct_blocked_identity.py already holds against the definition)"""
    need = F + F // 2
    for M in (2048, 4096, 6144, 8192):
        if need <= M:
            return M
    return 1 << int(np.ceil(np.log2(need)))


def bar2_of(v4, Cr, dCr, floor_columns=(ANTIPODAL,)):
    """bar 2 of the float32 transforms, per series of v4 (R, F, V, 3): EMU_FACTOR x max_t |emulate_f32 - oracle| / scale on these very
    chunks, never more than the north star.  The emulation restores the means in float64 where the kernels round x^2, y^2, z^2 and
    hold e[j] in float32, so on a series whose products are constant (floor_columns: antipodal) it is exact to 1e-13 and says
    nothing about a float32 implementation: there, and only there, the figure it multiplies is at least one float32 rounding of
    C(0) = 1, 2^-24.  Returns (bar per series, the emulation's error per series)."""
    R, F = v4.shape[:2]
    Ce, dCe = emulate_f32(v4, transform_points(F))
    emu, _ = errors(Ce, dCe, Cr, dCr, R)
    fig = emu.copy()
    for k in floor_columns:
        fig[k] = max(fig[k], EMU_FLOOR)
    return np.minimum(NORTH_STAR, EMU_FACTOR * fig), emu


def bar2(F):
    """bar2_of the chunks of case(F), computed once"""
    def make():
        vecs, R, Cr, dCr = case(F)
        return bar2_of(vecs[:R * F].reshape(R, F, 8, 3), Cr, dCr)
    return _once(('bar2', F), make)
