"""
GPU parity tests (run with -m gpu on an MI355X).  Every test calls the HIP path through the C ABI
(spinrelax_amd.hip.Context -> libspinrelax_hip.so) and checks it against
  * the committed golden vectors produced by the real reference (tests/golden/), and
  * the CPU oracle (oracle/) on the same seeded inputs.
Tolerances: integer work (histogram counts) bit-exact; floating point 1e-6 relative as BASELINE.json's
north_star states, written next to each assertion.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden, relerr, ct_f32_transform, dct_close_f32_transform
import sr_oracle as o
from spinrelax_amd import synth

pytestmark = pytest.mark.gpu

RTOL = 1e-6            # north_star: C(t), J(w), R1/R2/NOE within 1e-6 relative


@pytest.fixture(scope='module')
def ctx():
    from spinrelax_amd.hip import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def liboracle():
    so = os.path.join(ROOT, 'oracle', 'libsr_oracle.so')
    if not os.path.isfile(so):
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'oracle'), 'libsr_oracle.so'])
    lib = ctypes.CDLL(so)
    lib.sr_oracle_ct_palmer_f64.restype = ctypes.c_int
    return lib


def c_oracle_ct(lib, v4):
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


def dct_close(dCt, ref, R, F):
    """dC(t) = std over the R replicate means p_r / (sqrt(R) - 1).  The bar is set on the quantity the
    kernel computes, p_r: 1e-6 / sqrt(F/2) absolute (float32 rounding of the dot products, 1e-7 per term,
    averaged over F/2..F terms) -- i.e. well inside 1e-6 relative of C(t) -- and propagated through the
    std: |d dCt| <= that / (sqrt(R) - 1).  For scale: the reference's own float32 dC(t) is off by
    1e-4 .. 31 % relative and its _Ctint.dat keeps 8 decimals."""
    err = np.abs(dCt - ref)
    atol = 1e-6 / np.sqrt(F / 2.0) / (np.sqrt(R) - 1.0)
    return np.all(err <= np.maximum(RTOL * np.abs(ref), atol))


# ------------------------------------------------------------------------------------------------
# kernel 1: C(t)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,cfg,nvec', [('cfg1', 1, None), ('cfg2', 2, None), ('cfg3s', 3, 8)])
@pytest.mark.parametrize('mode', [0, 1])
def test_ct_vs_golden(ctx, synth_cache, tag, cfg, nvec, mode):
    g = golden('%s_ct.npz' % tag)
    s = synth.config_shapes(cfg)
    vecs = synth_cache(cfg, nvec)
    Ct, dCt = ctx.ct_palmer(vecs, s['R'], s['F'], mode=mode)
    assert Ct.shape == g['Ct64'].shape
    tol = RTOL if mode == 0 else 1e-12
    assert relerr(Ct, g['Ct64']) < tol
    if mode == 1:
        assert relerr(dCt, g['dCt64']) < 1e-9
    else:
        assert dct_close(dCt, g['dCt64'], s['R'], s['F'])
        # in practice the fast path is far inside the bar: record it
        assert relerr(Ct, g['Ct64']) < 1e-7


def test_ct_sharded_vector_range(ctx, synth_cache):
    """v0/nV select a shard of the vectors; results must equal the full run's columns."""
    s = synth.config_shapes(1)
    vecs = synth_cache(1)
    full, dfull = ctx.ct_palmer(vecs, s['R'], s['F'])
    part, dpart = ctx.ct_palmer(vecs, s['R'], s['F'], v0=5, nV=11)
    np.testing.assert_array_equal(part, full[:, 5:16])
    np.testing.assert_array_equal(dpart, dfull[:, 5:16])


@pytest.mark.parametrize('F,R,V', [(2, 3, 2), (3, 2, 1), (7, 4, 3), (64, 3, 5), (254, 2, 3), (255, 2, 3), (256, 2, 3),
                                   (257, 3, 2), (510, 2, 2), (1000, 2, 3), (1026, 2, 2), (100, 1, 2)])
def test_ct_ragged_and_edge_sizes(ctx, liboracle, F, R, V):
    """odd / tiny / just-around-a-lag-block chunk lengths, R = 1 (dCt = NaN like numpy), tail frames ignored"""
    vecs = synth.synth_vectors(R * F + 3, V, seed=100 + F)      # 3 trailing frames must be ignored
    v4 = vecs[:R * F].reshape(R, F, V, 3)
    Cr, dCr = c_oracle_ct(liboracle, v4)
    for mode in (0, 1):
        Ct, dCt = ctx.ct_palmer(vecs, R, F, mode=mode)
        assert Ct.shape == (F // 2, V)
        assert relerr(Ct, Cr) < RTOL
        if R == 1:
            assert np.all(np.isnan(dCt)) and np.all(np.isnan(dCr))
        else:
            assert dct_close(dCt, dCr, R, F)


@pytest.mark.parametrize('ct_fft', [3, 4, 2])
@pytest.mark.parametrize('F,R,V', [(683, 2, 3), (684, 2, 3), (1365, 3, 2), (1366, 2, 2), (2000, 2, 3), (2730, 2, 2), (2731, 2, 2),
                                   (3000, 2, 2), (4096, 2, 3), (4097, 2, 2), (5000, 2, 2), (5461, 2, 1), (5462, 2, 1)])
def test_ct_fft_formulation_all_transform_sizes(ctx, liboracle, F, R, V, ct_fft):
    """The FFT formulation of kernel 1 (default for 1024 < F + L <= 8192) at every transform size and on both sides of
    every switch: 2048 / 4096 / 8192 points, chunks that fill at most half of the transform (upper half skipped) and
    chunks that do not, the last length that fits (5461) and the first that falls back to the direct kernel (5462).
    Checked against the plain-C float64 oracle.  ct_fft = 2: float64 transforms everywhere, float64 accuracy.  ct_fft = 3 (the
    default): FLOAT32 transforms for 4096 < F + L <= 8192 (k_ct_rfft32: F = 2731 .. 5461 here), within the float32 bars; ct_fft = 4:
    float32 transforms at every transform length (M = 2048 and 4096 as well)."""
    vecs = synth.synth_vectors(R * F + 5, V, seed=300 + F)
    v4 = vecs[:R * F].reshape(R, F, V, 3)
    Cr, dCr = c_oracle_ct(liboracle, v4)
    ctx.set_option('ct_fft', ct_fft)
    try:
        Ct, dCt = ctx.ct_palmer(vecs, R, F)
        Ct1, dCt1 = ctx.ct_palmer(vecs, R, F, mode=1)            # the direct float64 mode
    finally:
        ctx.set_option('ct_fft', 3)
    assert Ct.shape == (F // 2, V)
    uses_fft = 1024 < F + F // 2 <= 8192
    if uses_fft and ct_f32_transform(F, ct_fft):
        assert relerr(Ct, Cr) < 1e-7 and dct_close_f32_transform(dCt, dCr, R)
        assert relerr(Ct, Ct1) < 1e-7
    else:
        assert relerr(Ct, Cr) < (1e-12 if uses_fft else RTOL)
        assert np.max(np.abs(dCt - dCr)) <= (1e-12 if uses_fft else 1e-6) * max(1.0, np.max(np.abs(dCr)))
        assert relerr(Ct, Ct1) < (1e-12 if uses_fft else RTOL)


def test_ct_rfft32_float32_transforms(ctx, liboracle):
    """k_ct_rfft32 (sr_ct32.hip), the production kernel of cfg3 / cfg4 (4096 < F + L <= 8192; shorter chunks with ct_fft = 4): float32 transforms of the mean-removed traceless
    components, mean terms restored in float64.  Against the plain-C float64 oracle on every path of the kernel: the aligned
    full-chunk form (F = 4096), masked chunks (F < 4096, odd F), the 8192-point transform, odd chunk starts (32-bit loads),
    series that are not unit vectors (the sixth signal |u|^2: scaled vectors, zero vectors of vecnorm_NDarray's 0/0 guard, one frame
    just outside the unit tolerance), constant vectors, and the series of one launch mixed.  Bars: C(t) 1e-7 relative (measured
    2-5e-8), dC(t) 5e-8 / (sqrt(R) - 1) absolute (conftest.dct_close_f32_transform)."""
    worst = 0.0
    ctx.set_option('ct_fft', 4)            # float32 transforms at every length (the default takes them for 4096 < F + L <= 8192)
    for F, R, V in ((4096, 3, 6), (4000, 3, 2), (3001, 3, 2), (2732, 4, 2), (4094, 2, 2), (4097, 3, 2), (5000, 3, 2), (5333, 2, 2), (5461, 2, 1),
                    (684, 3, 6), (1000, 4, 2), (1365, 3, 2), (1366, 3, 6), (2001, 3, 2), (2730, 2, 2), (2731, 2, 2)):       # M = 2048, 4096 too
        vecs = synth.synth_vectors(R * F + 7, V, seed=500 + F).copy()
        if V >= 2:
            vecs[:, 1] *= np.float32(1.7)                               # not unit: whole series scaled
        if V >= 6:
            vecs[100:140, 2] = 0.0                                      # a few zero vectors (0/0 guard)
            vecs[:, 3] *= (1.0 + 0.2 * np.sin(np.arange(vecs.shape[0]) / 50.0)).astype(np.float32)[:, None]
            vecs[F + 5, 4] *= np.float32(1.0 + 2e-6)                    # one frame of one chunk just outside the tolerance
        Cr, dCr = c_oracle_ct(liboracle, vecs[:R * F].reshape(R, F, V, 3))
        Ct, dCt = ctx.ct_palmer(vecs, R, F)
        e = relerr(Ct, Cr)
        worst = max(worst, e)
        assert e < 1e-7 and dct_close_f32_transform(dCt, dCr, R, Cr), (F, R, e, np.max(np.abs(dCt - dCr)))
    ctx.set_option('ct_fft', 3)
    print('\n[k_ct_rfft32] worst C(t) relative error over the shapes: %.2e' % worst)
    # odd chunk starts (two "files" whose first one has an odd number of frames)
    F = 4096
    a = synth.synth_vectors(2 * F + 1, 3, seed=78)
    b = synth.synth_vectors(F + 9, 3, seed=79)
    cat = np.ascontiguousarray(np.concatenate([a, b]))
    starts = np.array([0, F, 2 * F + 1], dtype=np.int64)
    Cr, dCr = c_oracle_ct(liboracle, np.stack([cat[st:st + F] for st in starts]))
    Ct, dCt = ctx.ct_palmer(cat, 3, F, chunk_start=starts)
    assert relerr(Ct, Cr) < 1e-7 and dct_close_f32_transform(dCt, dCr, 3)
    # constant unit vectors: every mean-removed signal is identically zero, C(t) = 1 comes out of the float64 mean terms alone
    const = np.zeros((2 * F, 3, 3), dtype=np.float32)
    const[:, 0, 0] = 1.0
    const[:, 1, 1] = 1.0
    const[:, 2, 2] = -1.0
    Ct4, dCt4 = ctx.ct_palmer(const, 2, F)
    assert np.max(np.abs(Ct4 - 1.0)) <= 4e-15 and np.max(np.abs(dCt4)) <= 4e-15
    # same answer as the float64 transform kernel on the cfg3 slice, to the float32 bar
    s = synth.config_shapes(3)
    v3 = synth.synth_config(3, nvec=8)
    C3, D3 = ctx.ct_palmer(v3, s['R'], s['F'])
    ctx.set_option('ct_fft', 2)
    try:
        C2, D2 = ctx.ct_palmer(v3, s['R'], s['F'])
    finally:
        ctx.set_option('ct_fft', 3)
    assert relerr(C3, C2) < 1e-7 and dct_close(D3, D2, s['R'], s['F'])


def test_ct_multi_file_chunk_starts(ctx, liboracle):
    """reformat_vecs_by_tau drops each file's tail separately (calculate-Ct-from-traj.py:259-272)."""
    from spinrelax_amd import ct as hostct
    a = synth.synth_vectors(700, 4, seed=11)
    b = synth.synth_vectors(530, 4, seed=12)
    F = 200
    v4 = o.reformat_vecs_by_tau([a, b], 1.0, float(F))
    cat, starts, R = hostct.concat_with_chunk_starts([a, b], F)
    assert R == v4.shape[0] == 5
    Ct, dCt = ctx.ct_palmer(cat, R, F, chunk_start=starts)
    Cr, dCr = c_oracle_ct(liboracle, v4)
    assert relerr(Ct, Cr) < RTOL and dct_close(dCt, dCr, R, F)
    # the same through the FFT formulation (chunk length 1200 -> 2048-point transforms)
    a = synth.synth_vectors(3900, 3, seed=13)
    b = synth.synth_vectors(2700, 3, seed=14)
    F = 1200
    v4 = o.reformat_vecs_by_tau([a, b], 1.0, float(F))
    cat, starts, R = hostct.concat_with_chunk_starts([a, b], F)
    assert R == v4.shape[0] == 5
    Ct, dCt = ctx.ct_palmer(cat, R, F, chunk_start=starts)
    Cr, dCr = c_oracle_ct(liboracle, v4)
    assert relerr(Ct, Cr) < 1e-12 and np.max(np.abs(dCt - dCr)) < 1e-12              # float64 transforms at this length (the default)
    ctx.set_option('ct_fft', 4)                                                     # float32 transforms
    try:
        Ct, dCt = ctx.ct_palmer(cat, R, F, chunk_start=starts)
    finally:
        ctx.set_option('ct_fft', 3)
    assert relerr(Ct, Cr) < 1e-7 and dct_close_f32_transform(dCt, dCr, R)


def test_ct_size_independent_properties(ctx):
    """Properties that hold at any size: rotation invariance, time reversal, constant vector -> C(t)=1."""
    s = synth.config_shapes(2)
    vecs = synth.synth_config(2, nvec=16)
    Ct, dCt = ctx.ct_palmer(vecs, s['R'], s['F'])
    # (1) a fixed rotation of every frame leaves P2(u.u') unchanged
    q = np.array([0.5, -0.5, 0.5, 0.5])
    rot = o.rotate_vector_simd(vecs, q).astype(np.float32)
    Ct2, _ = ctx.ct_palmer(rot, s['R'], s['F'])
    assert relerr(Ct2, Ct) < 5e-7          # inputs re-rounded to float32
    # (2) reversing time inside every chunk leaves the autocorrelation unchanged
    N = s['R'] * s['F']
    rev = vecs[:N].reshape(s['R'], s['F'], -1, 3)[:, ::-1].reshape(N, -1, 3)
    Ct3, _ = ctx.ct_palmer(np.ascontiguousarray(rev), s['R'], s['F'])
    assert relerr(Ct3, Ct) < 1e-7
    # (3) constant unit vectors: C(t) = 1, dCt = 0 -- exactly for the direct kernel (representable sums), to a few ulp
    #     for the FFT formulation the default mode uses at this chunk length
    const = np.zeros((N, 3, 3), dtype=np.float32)
    const[:, 0, 0] = 1.0
    const[:, 1, 1] = 1.0
    const[:, 2, 2] = -1.0
    Ct4, dCt4 = ctx.ct_palmer(const, s['R'], s['F'])
    assert np.max(np.abs(Ct4 - 1.0)) <= 4e-15 and np.max(np.abs(dCt4)) <= 4e-15
    ctx.set_option('ct_fft', 0)
    Ct5, dCt5 = ctx.ct_palmer(const, s['R'], s['F'])
    ctx.set_option('ct_fft', 3)          # the library default: later tests of this module run the production dispatch
    np.testing.assert_array_equal(Ct5, 1.0)
    np.testing.assert_array_equal(dCt5, 0.0)
    # (4) C(t) of a unit vector is bounded: -0.5 <= C <= 1
    assert Ct.max() <= 1.0 + 1e-12 and Ct.min() >= -0.5



def test_ct_rfft_traceless_form_and_its_fallback(ctx, liboracle):
    """k_ct_rfft<12> (4096 < F + L <= 6144, BASELINE cfg3's chunk length) runs FIVE transforms on the traceless components
    of u (x) u and takes the trace term |u|^2 |u'|^2 / 3 from prefix sums of |u|^2 - 1 when every vector of the series
    is a float32 unit vector; any other series (scaled vectors, the zero vectors vecnorm_NDarray's 0/0 guard produces)
    takes the sixth transform on |u|^2.  Both must agree with the plain-C float64 oracle at float64 accuracy, also with
    chunk starts that are odd (unaligned 8-byte pairs: the 32-bit load path) and with the series of one launch mixed."""
    ctx.set_option('ct_fft', 2)             # the float64 real-input kernel (the default dispatch runs k_ct_rfft32 at this length)
    ctx.set_option('ct_traceless', 1)
    try:
        F, R, V = 4096, 3, 6
        vecs = synth.synth_vectors(R * F + 7, V, seed=77).copy()
        vecs[:, 1] *= np.float32(1.7)                                   # not unit: whole series scaled
        vecs[100:140, 2] = 0.0                                          # a few zero vectors (0/0 guard)
        vecs[:, 3] *= (1.0 + 0.2 * np.sin(np.arange(vecs.shape[0]) / 50.0)).astype(np.float32)[:, None]
        vecs[F + 5, 4] *= np.float32(1.0 + 2e-6)                        # one frame of one chunk just outside the tolerance
        v4 = vecs[:R * F].reshape(R, F, V, 3)
        Cr, dCr = c_oracle_ct(liboracle, v4)
        Ct, dCt = ctx.ct_palmer(vecs, R, F)
        assert relerr(Ct, Cr) < 1e-12 and np.max(np.abs(dCt - dCr)) <= 1e-12 * max(1.0, np.max(np.abs(dCr)))
        # odd chunk starts (two "files" whose first one has an odd number of frames)
        a = synth.synth_vectors(2 * F + 1, 3, seed=78)
        b = synth.synth_vectors(F + 9, 3, seed=79)
        cat = np.ascontiguousarray(np.concatenate([a, b]))               # the odd tail of the first file stays in the array
        starts = np.array([0, F, 2 * F + 1], dtype=np.int64)
        v4 = np.stack([cat[st:st + F] for st in starts])
        Cr, dCr = c_oracle_ct(liboracle, v4)
        Ct, dCt = ctx.ct_palmer(cat, 3, F, chunk_start=starts)
        assert relerr(Ct, Cr) < 1e-12 and np.max(np.abs(dCt - dCr)) <= 1e-12
        # constant unit vectors at the production chunk length: C(t) = 1 to a few ulp, dC(t) = 0
        const = np.zeros((2 * F, 3, 3), dtype=np.float32)
        const[:, 0, 0] = 1.0
        const[:, 1, 1] = 1.0
        const[:, 2, 2] = -1.0
        Ct4, dCt4 = ctx.ct_palmer(const, 2, F)
        assert np.max(np.abs(Ct4 - 1.0)) <= 4e-15 and np.max(np.abs(dCt4)) <= 4e-15
        # shorter chunks of the same transform length (F = 3000: zero padding inside the loaded blocks)
        vecs = synth.synth_vectors(2 * 3000, 2, seed=80).copy()
        vecs[:, 1] *= np.float32(0.5)
        Cr, dCr = c_oracle_ct(liboracle, vecs.reshape(2, 3000, 2, 3))
        Ct, dCt = ctx.ct_palmer(vecs, 2, 3000)
        assert relerr(Ct, Cr) < 1e-12
        # the default (six-signal) kernel on the same input: the two forms agree to the accuracy of either
        ctx.set_option('ct_traceless', 0)
        Ct0, dCt0 = ctx.ct_palmer(vecs, 2, 3000)
        assert relerr(Ct0, Cr) < 1e-12 and relerr(Ct0, Ct) < 1e-12
    finally:
        ctx.set_option('ct_traceless', 0)
        ctx.set_option('ct_fft', 3)


def test_ct_rejects_bad_arguments(ctx):
    from spinrelax_amd.hip import SpinRelaxHipError
    vecs = synth.synth_vectors(100, 2, seed=1)
    with pytest.raises(SpinRelaxHipError):
        ctx.ct_palmer(vecs, 2, 100)                      # R*F exceeds the frames given
    with pytest.raises(SpinRelaxHipError):
        ctx.ct_palmer(vecs, 1, 1)                        # F < 2
    big = ctx.max_frames_per_chunk() + 64
    with pytest.raises(SpinRelaxHipError):
        ctx.ct_palmer(np.zeros((big, 1, 3), np.float32), 1, big)   # does not fit LDS: loud error, no fallback


# ------------------------------------------------------------------------------------------------
# kernel 2: rotate + histogram + mean vector + S2
# ------------------------------------------------------------------------------------------------
def s2_from_outer(outer, Fb):
    """calculate_S2_by_outerProduct (calculate-Ct-from-traj.py:133-142) from the per-block sums."""
    m = outer / Fb                                         # (nB, V, 6): xx yy zz xy xz yz
    s = 1.5 * (m[..., 0] ** 2 + m[..., 1] ** 2 + m[..., 2] ** 2 + 2 * (m[..., 3] ** 2 + m[..., 4] ** 2 + m[..., 5] ** 2)) - 0.5
    nB = s.shape[0]
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.stack((s.mean(axis=0), s.std(axis=0) / (np.sqrt(nB) - 1.0)), axis=-1)


@pytest.mark.parametrize('tag,cfg', [('cfg1', 1), ('cfg2', 2)])
def test_vechist_vs_golden(ctx, synth_cache, tag, cfg):
    g = golden('%s_vec.npz' % tag)
    s = synth.config_shapes(cfg)
    vecs = synth_cache(cfg)[: s['N']]
    hist, vecsum, outer = ctx.rotate_hist(vecs, g['q'], g['edges_phi'], g['edges_cos'], block_len=s['F'])
    # integer work: bit-exact
    np.testing.assert_array_equal(hist.astype(np.uint32), g['hist'])
    assert hist.sum() == g['hist_sum'] == s['N'] * s['V']
    avg = vecsum / s['N']
    avg = avg / np.sqrt((avg ** 2).sum(-1))[:, None]
    assert relerr(avg, g['avgvec']) < 1e-12
    assert relerr(s2_from_outer(outer, s['F']), g['S2_tau']) < 1e-9
    _, _, outer_all = ctx.rotate_hist(vecs, g['q'], g['edges_phi'], g['edges_cos'], block_len=0)
    m = outer_all[0] / s['N']
    S2all = 1.5 * (m[:, 0] ** 2 + m[:, 1] ** 2 + m[:, 2] ** 2 + 2 * (m[:, 3] ** 2 + m[:, 4] ** 2 + m[:, 5] ** 2)) - 0.5
    assert relerr(S2all, g['S2_all']) < 1e-12
    rot = ctx.rotate_vectors(vecs, g['q'])
    np.testing.assert_array_equal(rot[g['rot_idx_n'], g['rot_idx_v']], g['rot_sample'])


def test_vechist_edge_cases(ctx):
    """poles, the phi = +-pi seam, exact bin edges, zero vectors (NaN -> dropped like numpy), no rotation"""
    e = o.lambert_edges()
    v = np.array([[0, 0, 1], [0, 0, -1], [-1, 0, 0], [-1, -0.0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0],
                  [0, 0, 0], [0.6, 0.8, 0], [1e-30, 0, 1], [np.cos(np.pi / 36), np.sin(np.pi / 36), 0.5]], dtype=np.float32)
    vecs = np.ascontiguousarray(v[:, None, :])                  # (11 frames, 1 vector)
    hist, vecsum, outer = ctx.rotate_hist(vecs, None, e[0], e[1])
    ref, _ = o.lambert_histogram(vecs.astype(np.float64))
    np.testing.assert_array_equal(hist, ref)
    assert hist.sum() == 10                                     # the zero vector is dropped
    # identity quaternion given explicitly behaves the same
    hist2, _, _ = ctx.rotate_hist(vecs, [2.0, 0, 0, 0], e[0], e[1])
    np.testing.assert_array_equal(hist2, ref)
    # other resolutions (--histBin)
    for nphi in (8, 36, 90):
        ee = o.lambert_edges(nphi)
        vv = synth.synth_vectors(500, 3, seed=5)
        h, _, _ = ctx.rotate_hist(vv, synth.Q_EXT, ee[0], ee[1])
        r, _ = o.lambert_histogram(o.rotate_vector_simd(vv, np.array(synth.Q_EXT)), nphi)
        np.testing.assert_array_equal(h, r)


def test_vechist_full_size_properties(ctx):
    """cfg3-shaped slice: every frame lands in exactly one bin; rotating by q then by q^-1 restores the
    unrotated histogram."""
    s = synth.config_shapes(3)
    vecs = synth.synth_config(3, nvec=8)[: s['N']]
    e = o.lambert_edges()
    h0, vs0, _ = ctx.rotate_hist(vecs, None, e[0], e[1], block_len=s['F'])
    assert np.all(h0.sum(axis=(1, 2)) == s['N'])
    q = np.array(synth.Q_EXT)
    rot = ctx.rotate_vectors(vecs, q)
    qinv = q * np.array([1, -1, -1, -1])
    back = ctx.rotate_vectors(rot.astype(np.float32), qinv)
    assert np.max(np.abs(back - vecs)) < 5e-7


# ------------------------------------------------------------------------------------------------
# kernel 3a: J(omega), R1/R2/NOE/rho
# ------------------------------------------------------------------------------------------------
def relax_inputs(g):
    n = len(g['names'])
    zeta = float(g['zeta'])
    return n, zeta * g['S2'], zeta * g['C'], g['tau'], g['nComps'].astype(np.int32)


def old_api_consts(MHz, csa, n):
    B0 = o.B0_from_Hz(MHz * 1e6)
    om = o.omega_set(B0, 'ps')
    fcsa = o.factor_CSA(np.broadcast_to(np.asarray(csa, dtype=float), (n,)), B0)
    return om, o.factor_DD(), fcsa, 1e-12, o.GAMMA['1H'] / o.GAMMA['15N']


def test_jomega_ufunc_twin(ctx):
    import json
    k = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'known_answers.json')))['Jomega_outer']
    x = np.array(k['x'])[:, None]
    y = np.array(k['y'])[None, :]
    out = ctx.jomega(x, y)
    assert relerr(out, np.array(k['out'])) < 1e-15
    z = ctx.jomega(np.array([0.0, 1.0]), np.array([0.0, 0.0]))
    assert np.isnan(z[0]) and z[1] == 1.0                      # 0/0 like the C loop


def test_relax_old_api_vs_golden(ctx):
    g = golden('cfg1_relax.npz')
    n, S2, C, tau, K = relax_inputs(g)
    Dpar, Dperp = o.symmtop_from_iso(float(g['Diso']), float(g['Dani']))
    for fi, MHz in enumerate(g['fields']):
        om, fdd, fcsa, tf, gr = old_api_consts(MHz, -170e-6, n)
        out, J = ctx.relax(1, [float(g['Diso'])], om, fdd, fcsa, tf, gr, S2, C, tau, K, want_J=True)
        assert relerr(out[0, :, :, 0].T, g['iso_f64_%d' % fi]) < 1e-12     # float64 values of the reference
        assert relerr(J[0, :, :, 0], g['iso_J_%d' % fi]) < 1e-12
        # and what the reference finally writes: its float32 datablock
        np.testing.assert_allclose(out[0, :, :, 0].T.astype(np.float32), g['iso_f32_%d' % fi], rtol=2e-7)
        for nm, csa in (('sym', -170e-6), ('symcsa', g['csa_alt'])):
            om, fdd, fcsa, tf, gr = old_api_consts(MHz, csa, n)
            out, J = ctx.relax(2, [Dpar, Dperp], om, fdd, fcsa, tf, gr, S2, C, tau, K,
                               binvecs=g['binvecs'], weights=g['weights'], noe_mode=0, want_J=True)
            ref = g['%s_f64_%d' % (nm, fi)]                                  # (4, n, 2)
            got = np.transpose(out[0], (1, 0, 2))
            assert relerr(got[..., 0], ref[..., 0]) < 1e-11                  # weighted means
            assert relerr(got[..., 1], ref[..., 1]) < 1e-8                   # weighted sigmas
            np.testing.assert_allclose(got.astype(np.float32), g['%s_f32_%d' % (nm, fi)], rtol=3e-7)
        # one vector per residue (calculate-relaxations-from-Ct.py:177-187)
        om, fdd, fcsa, tf, gr = old_api_consts(MHz, -170e-6, n)
        out, _ = ctx.relax(2, [Dpar, Dperp], om, fdd, fcsa, tf, gr, S2, C, tau, K, resvecs=g['sym1_vecs'])
        np.testing.assert_allclose(out[0, :, :, 0].T.astype(np.float32), g['sym1_f32_%d' % fi], rtol=3e-7)
        assert np.all(out[..., 1] == 0)


def test_relax_new_api_vs_golden(ctx):
    """class API: NOE from the vector-averaged R1 (spectral_densities.py:881-892); all 9 experiments at once"""
    g = golden('cfg1_relax.npz')
    n = len(g['names'])
    zeta = float(g['zeta'])
    S2, C, tau, K = zeta * g['S2'], zeta * g['C'], g['tau'], g['nComps'].astype(np.int32)
    Dpar, Dperp = o.symmtop_from_iso(float(g['Diso']), float(g['Dani']))
    oms, fcs = [], []
    for MHz in g['fields']:
        om, B0 = o.omega_set_new(MHz)
        oms.append(om)
        fcs.append(np.repeat(2.0 / 15.0 * (-170e-6) ** 2.0 * (o.GAMMA['15N'] * B0) ** 2, n))
    out, _ = ctx.relax(2, [Dpar, Dperp], np.array(oms), o.factor_DD_new(), np.array(fcs), 1e-12,
                       o.GAMMA['1H'] / o.GAMMA['15N'], S2, C, tau, K, binvecs=g['binvecs'], weights=g['weights'], noe_mode=1)
    for fi in range(3):
        for qi, kind in enumerate(('R1', 'R2', 'NOE')):
            assert relerr(out[fi, :, qi, 0], g['new_%s_val_%d' % (kind, fi)]) < 1e-11
            assert relerr(out[fi, :, qi, 1], g['new_%s_err_%d' % (kind, fi)]) < 1e-8
    # old and new NOE differ by design: make sure both modes are really different code
    out0, _ = ctx.relax(2, [Dpar, Dperp], np.array(oms), o.factor_DD_new(), np.array(fcs), 1e-12,
                        o.GAMMA['1H'] / o.GAMMA['15N'], S2, C, tau, K, binvecs=g['binvecs'], weights=g['weights'], noe_mode=0)
    assert 1e-6 < relerr(out0[:, :, 2, 0], out[:, :, 2, 0]) < 1e-2
    np.testing.assert_array_equal(out0[:, :, :2], out[:, :, :2])


def test_relax_known_answer_rigid_sphere(ctx):
    """--theoretical known answer: rigid sphere, S2 = zeta, no internal motion."""
    om, fdd, fcsa, tf, gr = old_api_consts(600.133, -170e-6, 1)
    out, _ = ctx.relax(1, [3.7383e-5], om, fdd, fcsa, tf, gr, [0.890023], [[0.0]], [[99999.0]], [1])
    assert abs(out[0, 0, 0, 0] / 2.216697349136826 - 1) < 1e-13
    assert abs(out[0, 0, 1, 0] / 6.743109911585374 - 1) < 1e-13
    assert abs(out[0, 0, 2, 0] / 0.7864966280916813 - 1) < 1e-13
    # direct transform model (no global tumbling)
    out, J = ctx.relax(0, None, om, fdd, fcsa, tf, gr, [0.8], [[0.1, 0.1]], [[50.0, 900.0]], [2], want_J=True)
    assert relerr(J[0, 0, :, 0], o.J_direct_transform(om, [0.1, 0.1], [50.0, 900.0])) < 1e-14


# ------------------------------------------------------------------------------------------------
# kernel 3b: multi-exponential model, device TRF fit
# ------------------------------------------------------------------------------------------------
def test_resjac_vs_oracle_and_reference_chi(ctx):
    g = golden('cfg2_fit.npz')
    t, y, dy = g['t'], g['y'], g['dy']
    for j, nP in enumerate(g['listDoG']):
        ok = g['trial_quality'][:, j, 0]
        p = g['trial_popt'][ok, j, :nP]
        resid, jac = ctx.expfit_resjac(t[ok], y[ok], dy[ok], p)
        for i in range(p.shape[0]):
            model = o.curvefit_exponential(t[ok][i], *p[i])
            assert relerr(resid[i] * dy[ok][i] + y[ok][i], model) < 1e-13
            # chi^2 of the reference at the reference's optimum (tier (i) of the fit parity contract)
            chi = np.mean((resid[i] * dy[ok][i]) ** 2 / dy[ok][i])
            assert abs(chi / g['trial_chi'][ok][i, j] - 1) < 1e-9
        # analytic Jacobian vs central differences of the oracle model
        i = 0
        for k in range(nP):
            h = 1e-6 * max(1.0, abs(p[i, k]))
            pp, pm = p[i].copy(), p[i].copy()
            pp[k] += h
            pm[k] -= h
            fd = (o.curvefit_exponential(t[ok][i], *pp) - o.curvefit_exponential(t[ok][i], *pm)) / (2 * h) / dy[ok][i]
            assert np.max(np.abs(jac[i, :, k] - fd)) <= 1e-6 * max(1.0, np.max(np.abs(fd)))


@pytest.mark.parametrize('tag', ['cfg1', 'cfg2', 'cfg3s'])
def test_device_fit_vs_reference_trials(ctx, tag):
    """Every (residue, model order) trial of the fixtures, started from the reference's own p0.

    The device solver restates scipy's TRF step for step (sr_fit.hip) and normally needs exactly the same number of
    function evaluations.  The bar is per trial:  |chi^2 / chi^2_ref - 1| <= 1e-6 for orders of up to 5 parameters and
    <= 1e-4 for the over-parameterised 7 / 9-parameter orders -- unless the REFERENCE ITSELF does not pin its answer that
    well: tests/golden/<tag>_fit_sens.npz (oracle/gen_golden_fit_sensitivity.py) holds, for every trial, the chi^2 values
    the real reference reaches when its input C(t) changes by ONE ulp (64 / 32 / 16 perturbed runs per trial; the size of
    change a different exp() or summation order makes).  ftol = xtol = 1e-8 stop a TRF run ~1e-4 from the stationary point
    along flat directions, so at L = 50 (cfg1) the reference's own 9-parameter chi^2 moves by up to 150 %, its 7-parameter
    fit of residue 26 jumps to a minimum 24 % higher in 2 of 64 runs (the one the device lands in), and even its
    2-parameter fits move by 1.7e-6; at L >= 512 everything up to 7 parameters is stable to 2e-5 or better.
      * every trial the reference pins ten times better than the tier must meet the tier;
      * any other trial must meet the tier, OR lie inside the reference's own range of outcomes (widened by half its width),
        OR deviate by no more than three times the reference's own largest deviation: the perturbed runs sample what the
        reference does under one-ulp changes, they do not bound it.
    Failures of the reference are reproduced (same residues fail)."""
    g = golden('%s_fit.npz' % tag)
    sens = golden('%s_fit_sens.npz' % tag)
    t, y, dy = g['t'], g['y'], g['dy']
    nres = y.shape[0]
    tau_max = t[0, -1] * 10
    stats = {}
    for j, nP in enumerate(g['listDoG']):
        p0 = g['trial_p0'][:, j, :nP]
        popt, pcov, chi, status, nfev = ctx.expfit(t, y, dy, p0, tau_max)
        K = nP // 2
        tier = 1e-6 if nP <= 5 else 1e-4
        n = within = pinned = over = mismatch = 0
        worst = 0.0
        for i in range(nres):
            ref_ok = bool(g['trial_quality'][i, j, 0])
            # success / failure must agree with the reference for EVERY order (7 and 9 parameters included), unless the
            # reference itself flips between success and failure under a one-ulp change of its input (trial_ok_flip)
            if (status[i] > 0) != ref_ok and not bool(sens['trial_ok_flip'][i, j]):
                mismatch += 1
            assert mismatch == 0, (tag, nP, i, status[i], ref_ok)
            if not ref_ok or status[i] <= 0:
                continue
            rel = abs(chi[i] / g['trial_chi'][i, j] - 1)
            spread = float(sens['trial_chi_spread'][i, j])
            assert np.all(popt[i, :K] >= 0) and np.all(popt[i, :K] <= 1) and np.all(popt[i, K:2 * K] <= tau_max)
            n += 1
            within += rel <= tier
            if spread <= 0.1 * tier:
                pinned += 1
                assert rel <= tier, (tag, nP, i, rel, spread)                 # the reference pins it: so must the device
            elif rel > tier:
                over += 1
                lo, hi = float(sens['trial_chi_lo'][i, j]), float(sens['trial_chi_hi'][i, j])
                inside = lo * (1 - tier) - 0.5 * (hi - lo) <= chi[i] <= hi * (1 + tier) + 0.5 * (hi - lo)
                assert inside or rel <= 3.0 * spread, (tag, nP, i, rel, spread, chi[i], lo, hi)
            worst = max(worst, rel)
        stats[int(nP)] = dict(fits=int(n), within_tier=int(within), pinned=int(pinned), beyond_tier=int(over),
                              status_mismatch=int(mismatch), worst=float(worst))
    print('\n[fit trials %s] order: fits, within tier, pinned by the reference (all within tier), beyond tier where the reference itself moves, '
          'status mismatches, worst' % tag)
    for nP, e in stats.items():
        print('   %d parameters: %3d, %3d, %3d, %3d, %d, %.1e' % (nP, e['fits'], e['within_tier'], e['pinned'], e['beyond_tier'], e['status_mismatch'], e['worst']))
    # The tallies are part of the contract (tests/golden/fit_trial_tallies.json, measured on MI355X): a change that moves
    # trials from "within tier" to "inside the reference's own spread" must not stay green.  The solver is deterministic
    # (fixed-order reductions), so the counts are exact; `worst` gets 1 % of slack.
    from conftest import committed_tally
    want = committed_tally('fit_trials', tag, {str(k): v for k, v in stats.items()})
    for nP, e in stats.items():
        w = want[str(nP)]
        assert e['fits'] == w['fits'] and e['pinned'] == w['pinned'], (tag, nP, e, w)
        assert e['within_tier'] >= w['within_tier'] and e['beyond_tier'] <= w['beyond_tier'], (tag, nP, e, w)
        assert e['status_mismatch'] <= w['status_mismatch'], (tag, nP, e, w)
        assert e['worst'] <= w['worst'] * 1.01 + 1e-12, (tag, nP, e, w)


def test_fit_uniform_grid_products_and_the_fallback(ctx):
    """exp(-t/tau) on a uniform time grid: the fit kernels multiply along a thread's points instead of calling exp() per point
    (option fit_geo, default on; sr_fit.hip Residue::stage decides per residue on the device).  (1) against exp() per point
    (fit_geo = 0) on the reference's cfg2 / cfg3 trial inputs: the well-conditioned orders (2, 3, 5 parameters) end on the same
    minimum to what ftol = xtol = 1e-8 leave of it -- chi^2 to the 1e-6 tier of test_device_fit_vs_reference_trials (measured
    1e-7: the reference's own chi^2 moves as much under a one-ulp change of its input), parameters to 1e-5 of their scale; (2) an axis that is NOT a uniform grid (one time moved by 1e-9
    of itself; a quadratic axis) takes exp() per point whatever the option says: bit-identical results with fit_geo = 1 and 0;
    (3) L <= 256 (cfg1: one point per thread) is the exp() path by construction: bit-identical as well.
    (4) the over-parameterised orders (7, 9 parameters), where one ulp of input moves the reference itself by more than any tier:
    with either form every trial succeeds or fails as the reference does (unless the reference itself flips under a one-ulp change
    of its input, <tag>_fit_sens.npz), and every chi^2 meets the 1e-4 tier of test_device_fit_vs_reference_trials or lies inside the
    reference's own range of outcomes by that test's rule."""
    for tag in ('cfg2', 'cfg3s'):
        g = golden('%s_fit.npz' % tag)
        sens = golden('%s_fit_sens.npz' % tag)
        t, y, dy = g['t'], g['y'], g['dy']
        tau_max = t[0, -1] * 10
        for j, nP in enumerate(g['listDoG']):
            p0 = g['trial_p0'][:, j, :nP]
            out = {}
            for geo in (1, 0):
                ctx.set_option('fit_geo', geo)
                out[geo] = ctx.expfit(t, y, dy, p0, tau_max)
            ctx.set_option('fit_geo', 1)
            if nP > 5:
                tier = 1e-4
                for geo in (1, 0):
                    chi, status = out[geo][2], out[geo][3]
                    n_tier = n_spread = 0
                    for i in range(y.shape[0]):
                        ref_ok = bool(g['trial_quality'][i, j, 0])
                        assert (status[i] > 0) == ref_ok or bool(sens['trial_ok_flip'][i, j]), (tag, nP, geo, i, status[i])
                        if not ref_ok or status[i] <= 0:
                            continue
                        rel = abs(chi[i] / g['trial_chi'][i, j] - 1)
                        spread = float(sens['trial_chi_spread'][i, j])
                        lo, hi = float(sens['trial_chi_lo'][i, j]), float(sens['trial_chi_hi'][i, j])
                        inside = lo * (1 - tier) - 0.5 * (hi - lo) <= chi[i] <= hi * (1 + tier) + 0.5 * (hi - lo)
                        assert rel <= tier or (spread > 0.1 * tier and (inside or rel <= 3.0 * spread)), \
                            (tag, nP, geo, i, rel, spread, chi[i], lo, hi)
                        n_tier += rel <= tier
                        n_spread += rel > tier
                    print('\n[fit_geo %s, %d parameters, geo=%d] within the tier %d, inside the reference\'s spread %d'
                          % (tag, nP, geo, n_tier, n_spread))
                continue
            ok = (out[1][3] > 0) & (out[0][3] > 0)
            assert np.array_equal(out[1][3] > 0, out[0][3] > 0) and ok.sum() >= 0.75 * len(ok)
            chi_rel = np.max(np.abs(out[1][2][ok] / out[0][2][ok] - 1.0))
            scale = np.maximum(np.abs(out[0][0][ok]), 1e-3 * np.max(np.abs(out[0][0][ok]), axis=0))
            p_rel = np.max(np.abs(out[1][0][ok] - out[0][0][ok]) / scale)
            print('\n[fit_geo %s, %d parameters] chi^2 %.1e, parameters %.1e' % (tag, nP, chi_rel, p_rel))
            assert chi_rel < 1e-6 and p_rel < 1e-5, (tag, nP, chi_rel, p_rel)
    g = golden('cfg2_fit.npz')
    t, y, dy = g['t'].copy(), g['y'], g['dy']
    p0 = g['trial_p0'][:, 1, :3]
    for kind in ('moved', 'quadratic'):
        t2 = t.copy()
        if kind == 'moved':
            t2[:, 300] *= 1.0 + 1e-9
        else:
            t2 = t2 * (1.0 + 1e-3 * t2 / t2[:, -1:])
        res = []
        for geo in (1, 0):
            ctx.set_option('fit_geo', geo)
            res.append(ctx.expfit(t2, y, dy, p0, t2[0, -1] * 10))
        ctx.set_option('fit_geo', 1)
        for a, b in zip(res[0], res[1]):
            assert np.array_equal(a, b, equal_nan=True), kind
    g = golden('cfg1_fit.npz')
    res = []
    for geo in (1, 0):
        ctx.set_option('fit_geo', geo)
        res.append(ctx.expfit(g['t'], g['y'], g['dy'], g['trial_p0'][:, 0, :2], g['t'][0, -1] * 10))
    ctx.set_option('fit_geo', 1)
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('W', [1, 2, 4])
def test_fit_uniform_grid_lengths_and_wave_counts_vs_scipy(ctx, W):
    """The uniform-grid form at chunk lengths around the thread count (64 W threads per residue: L = 64 W + 1 gives one thread two
    points and the others one; L not a multiple of it; L below it takes exp() per point), for every wave count, a non-zero time
    origin, with and without sigma: a clean three-parameter decay with mild noise, fitted from the same start by scipy's
    curve_fit (what the reference calls, fitting_Ct_functions.py:322) -- parameters to 1e-6, and fit_geo = 0 agrees as well."""
    from scipy.optimize import curve_fit
    rng = np.random.RandomState(5 + W)
    ctx.set_option('fit_waves', W)
    try:
        for L in (64 * W - 3, 64 * W + 1, 64 * W * 2 + 37, 1000):
            for t0, with_sigma in ((0.0, True), (3.5, False)):
                t = t0 + 2.0 * np.arange(L)
                tau_true = 0.2 * t[-1]
                y = 0.85 + 0.15 * np.exp(-t / tau_true) + 1e-4 * rng.standard_normal(L)
                dy = np.full(L, 1e-3) if with_sigma else None
                p0 = np.array([[0.5, 0.1 * t[-1], 0.5]])
                tau_max = 10 * t[-1]

                def model(tt, C, tau, S2):
                    return S2 + C * np.exp(-tt / tau)
                ref, _ = curve_fit(model, t, y, sigma=dy, p0=p0[0], bounds=(0, [1.0, tau_max, 1.0]))
                for geo in (1, 0):
                    ctx.set_option('fit_geo', geo)
                    popt, pcov, chi, status, nfev = ctx.expfit(t[None], y[None], None if dy is None else dy[None], p0, tau_max)
                    assert status[0] > 0
                    err = np.max(np.abs(popt[0] / ref - 1.0))
                    assert err < 1e-6, (W, L, t0, with_sigma, geo, popt[0], ref)
    finally:
        ctx.set_option('fit_geo', 1)
        ctx.set_option('fit_waves', 2)


def test_device_fit_failure_modes(ctx):
    """p0 outside the bounds -> scipy raises ValueError, the reference marks the fit failed
    (fitting_Ct_functions.py:325-328); NaN data -> residuals not finite."""
    t = np.arange(1, 51) * 10.0
    y = 0.8 + 0.2 * np.exp(-t / 100.0)
    popt, pcov, chi, status, nfev = ctx.expfit(t, np.stack([y, y]), None, [[0.2, 100.0, 1.5], [0.2, 100.0, 0.8]], 5000.0)
    assert status[0] == -2 and np.isinf(chi[0])
    assert status[1] > 0 and abs(popt[1, 2] - 0.8) < 1e-6 and abs(popt[1, 1] - 100.0) < 1e-3
    yy = y.copy()
    yy[3] = np.nan
    _, _, chi, status, _ = ctx.expfit(t, yy[None], None, [[0.2, 100.0, 0.8]], 5000.0)
    assert status[0] == -3


def _host_driven_search(fitCt, t, y, dy, orders, ctx):
    search = fitCt.OrderSearchBatch(t, y, orders, 0.5)
    runner = fitCt.host_runner(t, y, dy, ctx=ctx)
    while True:
        req = search.request()
        if req is None:
            break
        search.submit(*runner(req['nParams'], req['p0'], req['idx']))
    return search


@pytest.mark.parametrize('tag', ['cfg1', 'cfg2', 'cfg3s'])
def test_device_order_search_equals_host_driven_search(ctx, tag):
    """The one-launch model-order search (sr_expfit_order_search_f64: guesses, fits, quality flags and accept/reject
    on the GPU) against the host-driven state machine OrderSearchBatch, which mirrors
    optimised_curve_fitting (fitting_Ct_functions.py:278-304) and is itself checked against the reference's
    selections in tests/test_formats_and_hostlogic.py.  Both drive the same device solver from the same initial
    guesses, so everything must agree bit for bit: selection, parameters, chi^2, evaluation counts."""
    from spinrelax_amd import fitting_Ct_functions as fitCt
    g = golden('%s_fit.npz' % tag)
    t, y, dy = g['t'], g['y'], g['dy']
    orders = tuple(int(v) for v in g['listDoG'])
    dev = fitCt.order_search_device(t, y, dy, orders, 0.5, ctx=ctx)
    search = _host_driven_search(fitCt, t, y, dy, orders, ctx)
    assert np.array_equal(dev['best'], search.best)
    # initial guesses: the p0 the reference itself used for every trial (first K amplitudes and the taus)
    for j, res in enumerate(search.per_order):
        nP = res['nParams']
        tried = dev['status'][j] != -100
        host_tried = ~np.isnan(res['p0'][:, 0])
        assert np.array_equal(tried, host_tried)
        idx = np.flatnonzero(tried)
        assert np.array_equal(dev['popt'][j][idx, :nP], res['popt'][idx])
        assert np.array_equal(dev['dP'][j][idx, :nP], res['dP'][idx], equal_nan=True)
        assert np.array_equal(dev['chisq'][j][idx], res['chiSq'][idx])
    S2, C, tau, K, chi = search.selected_arrays(Kmax=max(orders) // 2)
    assert np.array_equal(dev['K'], K)
    assert np.array_equal(dev['S2'], S2) and np.array_equal(dev['C'], C) and np.array_equal(dev['tau'], tau)
    assert np.array_equal(dev['chi'], chi, equal_nan=True)
    # and the reference's own selection (number of parameters of the accepted model) where its fits are stable
    ref_best = g['sel_nParams'] if 'sel_nParams' in g else None
    if ref_best is not None:
        mine = np.where(dev['best'] >= 0, np.asarray(orders)[np.maximum(dev['best'], 0)], 0)
        agree = int(np.sum(mine == ref_best))
        print('%s: selected order equals the reference for %d of %d residues' % (tag, agree, mine.size))
        from conftest import committed_tally
        want = committed_tally('order_agreement', tag, {'agree': agree, 'of': int(mine.size)})
        assert mine.size == want['of'] and agree >= want['agree'], (tag, agree, want)    # committed count, measured on MI355X


def test_device_order_search_edge_cases(ctx):
    """Short series (fewer than 10 lags: the means of initialise_for_fit_advanced shrink), a residue the first order
    already fails on (NaN), per-residue time axes, and L too long for LDS (global-memory path)."""
    from spinrelax_amd import fitting_Ct_functions as fitCt
    rng = np.random.default_rng(3)
    for L in (7, 64, 9000):
        t = np.arange(1, L + 1) * 10.0
        n = 5
        S2 = rng.uniform(0.3, 0.9, n)
        y = S2[:, None] + (1 - S2[:, None]) * np.exp(-t[None, :] / rng.uniform(50, 500, n)[:, None])
        y += 1e-4 * rng.standard_normal(y.shape)
        y[2, min(3, L - 1)] = np.nan
        dy = np.full_like(y, 1e-3)
        tt = np.ascontiguousarray(np.broadcast_to(t, y.shape))
        dev = fitCt.order_search_device(tt, y, dy, (2, 3, 5), 0.5, ctx=ctx)
        search = _host_driven_search(fitCt, tt, y, dy, (2, 3, 5), ctx)
        assert np.array_equal(dev['best'], search.best), L
        assert dev['best'][2] == -1 and dev['K'][2] == 0
        S2h, Ch, tauh, Kh, chih = search.selected_arrays(Kmax=2)
        assert np.array_equal(dev['S2'], S2h) and np.array_equal(dev['C'], Ch) and np.array_equal(dev['tau'], tauh)


@pytest.mark.parametrize('N,Vtot,v0,nV,Npad', [
    (1000, 32, 0, 32, 1024),          # one full tile column, last tile of frames partly past N
    (1001, 50, 7, 37, 1280),          # nothing aligned: odd Vtot, odd first vector, 37 vectors (32 + 5), N % 4 = 1
    (64, 3, 1, 1, 64),                # one vector
    (130, 96, 32, 64, 192),           # two full vector tiles of a larger array (the register kernel, padding inside its tile)
    (100, 64, 32, 32, 128),           # fewer frames than one tile of the register kernel
    (4099, 33, 0, 33, 4352),          # padding of more than one tile of frames behind N: written as zeros
])
def test_pack_planes_bit_exact(ctx, N, Vtot, v0, nV, Npad):
    """kernel 0 alone (sr_pack_soa_f32_dev): the planes are the vectors transposed, bit for bit, and every frame in [N, Npad) is
    zero -- for whole aligned 32-vector tiles (k_pack_soa, registers) and for shapes that are not multiples of a tile or of four
    (k_pack_soa_ragged, LDS tile)."""
    import torch
    rng = np.random.default_rng(N + Vtot)
    vecs = rng.standard_normal((N, Vtot, 3)).astype(np.float32)
    dev = torch.device('cuda', 0)
    d = torch.from_numpy(vecs).to(dev)
    soa = torch.full((nV, 3, Npad), float('nan'), device=dev, dtype=torch.float32)
    ctx.set_stream(0)
    ctx.pack_soa_dev(d.data_ptr(), N, Vtot, v0, nV, soa.data_ptr(), Npad)
    torch.cuda.synchronize()
    planes = soa.cpu().numpy()
    assert np.array_equal(planes[:, :, :N], np.transpose(vecs[:, v0:v0 + nV], (1, 2, 0)))
    assert not planes[:, :, N:].any()


def test_per_frame_rotation_and_fused_detumbling(ctx):
    """SURVEY.md section 8(f)-1.  (a) sr_rotate_vectors_perframe_f32 against the reference's rotate_vector_simd run bond
    by bond with one quaternion per frame; (b) the de-tumbling folded into the pack kernel
    (sr_pack_soa_rot_f32_dev) followed by the C(t) kernel against the reference's C(t) of the de-tumbled vectors."""
    import torch
    from spinrelax_amd import ct as hostct
    g = golden('cfg1_detumble.npz')
    lab = g['lab']
    qinv = g['q32'].astype(np.float64)
    qinv[:, 1:] *= -1.0
    rot = hostct.rotate_vector_simd(lab, qinv[:, None, :], ctx=ctx)
    assert rot.dtype == np.float64
    assert np.max(np.abs(rot[:, :8] - g['body64'])) <= 2.3e-16          # one ulp of a unit vector component
    body32 = hostct.detumble_vectors(lab, g['q32'], ctx=ctx)
    assert body32.dtype == np.float32 and np.array_equal(body32, rot.astype(np.float32))
    with pytest.raises(ValueError):
        hostct.detumble_vectors(lab, g['q32'][:10], ctx=ctx)
    # fused: planes straight from the lab-frame vectors + quaternions in HBM
    s = dict(R=10, F=100, L=50)
    N, V = lab.shape[:2]
    dev = torch.device('cuda', 0)
    dlab = torch.from_numpy(lab).to(dev)
    dq = torch.from_numpy(hostct.vecnorm_NDarray(qinv)).to(dev)
    Npad = (N + 63) // 64 * 64
    soa = torch.zeros((V, 3, Npad), device=dev, dtype=torch.float32)
    Ct = torch.empty((s['L'], V), device=dev, dtype=torch.float64)
    dCt = torch.empty_like(Ct)
    ctx.set_stream(0)
    ctx.pack_soa_rot_dev(dlab.data_ptr(), N, V, 0, V, dq.data_ptr(), soa.data_ptr(), Npad)
    ctx.ct_palmer_dev(soa.data_ptr(), Npad, s['R'], s['F'], V, Ct.data_ptr(), dCt.data_ptr())
    torch.cuda.synchronize()
    planes = soa.cpu().numpy()[:, :, :N]
    assert np.array_equal(np.transpose(planes, (2, 0, 1)), body32)
    assert relerr(Ct.cpu().numpy(), g['Ct64']) < 1e-12
    assert np.allclose(dCt.cpu().numpy(), g['dCt64'], rtol=1e-9, atol=1e-15)
