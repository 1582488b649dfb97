"""
GPU tests of C(t) for chunks longer than one in-LDS transform (F + L > 8192, up to 262144 frames per chunk): the blocked
Wiener-Khinchin kernels of spinrelax_amd/csrc/sr_ct_long.hip behind the default dispatch.  Yardstick: the plain-C float64
oracle (oracle/libsr_oracle.so).  Bars: the project's own for float32 transforms -- C(t) 1e-7 relative, dC(t) by
conftest.dct_close_f32_transform.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, relerr, dct_close_f32_transform
import sr_oracle as o
from spinrelax_amd import synth

pytestmark = pytest.mark.gpu

LIMIT = 262144
MIN_DEFAULT = 16384       # default of "ct_long_min_frames": chunks the direct kernel can stage (about 13 400 frames) stay with it


@pytest.fixture(scope='module')
def ctx():
    from spinrelax_amd.hip import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture
def blocked(ctx):
    """the blocked kernels also for the chunks the direct kernel could stage (5462 <= F <= about 13 400)"""
    ctx.set_option('ct_long_min_frames', 5462)
    yield ctx
    ctx.set_option('ct_long_min_frames', MIN_DEFAULT)


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


@pytest.mark.parametrize('F,R,V', [(5462, 3, 2), (8192, 2, 2), (8193, 3, 2), (10000, 3, 2), (12288, 2, 2), (13001, 3, 2), (16384, 2, 2),
                                   (21845, 3, 2), (25000, 2, 2), (40000, 2, 2), (100000, 2, 1), (262144, 2, 1)])
def test_ct_long_length_sweep(ctx, liboracle, F, R, V):
    """default dispatch at every length from the first that does not fit one transform to the limit (three trailing frames ignored);
    above the direct kernel's LDS limit (about 13 400 frames) these lengths used to be refused.  Below it the default is still
    the direct kernel; test_ct_long_blocked_below_direct_limit runs the blocked kernels there."""
    vecs = synth.synth_vectors(R * F + 3, V, seed=700 + F % 1000)
    Cr, dCr = c_oracle_ct(liboracle, vecs[:R * F].reshape(R, F, V, 3))
    Ct, dCt = ctx.ct_palmer(vecs, R, F)
    e = relerr(Ct, Cr)
    print('\n[ct_long] F=%d R=%d V=%d: C(t) relative error %.2e, dC(t) absolute error %.2e' % (F, R, V, e, np.max(np.abs(dCt - dCr))))
    assert e < 1e-7, (F, e)
    assert dct_close_f32_transform(dCt, dCr, R, Cr), (F, np.max(np.abs(dCt - dCr)))


@pytest.mark.parametrize('F,R,V', [(5462, 3, 2), (8192, 2, 2), (8193, 3, 2), (10000, 3, 2), (12288, 2, 2), (13001, 3, 2)])
def test_ct_long_blocked_below_direct_limit(blocked, liboracle, F, R, V):
    """the sweep's lengths that the direct kernel can stage too, through the blocked kernels ("ct_long_min_frames" = 5462)"""
    vecs = synth.synth_vectors(R * F + 3, V, seed=700 + F % 1000)
    Cr, dCr = c_oracle_ct(liboracle, vecs[:R * F].reshape(R, F, V, 3))
    Ct, dCt = blocked.ct_palmer(vecs, R, F)
    e = relerr(Ct, Cr)
    print('\n[ct_long blocked] F=%d R=%d V=%d: C(t) relative error %.2e, dC(t) absolute error %.2e' % (F, R, V, e, np.max(np.abs(dCt - dCr))))
    assert e < 1e-7, (F, e)
    assert dct_close_f32_transform(dCt, dCr, R, Cr), (F, np.max(np.abs(dCt - dCr)))


@pytest.mark.parametrize('F', [10000, 25000])
def test_ct_long_series_kinds(blocked, liboracle, F):
    """unit, scaled, zero-vector, modulated-norm and just-outside-the-tolerance series in one launch (the perturbations of
    test_ct_rfft32_float32_transforms), constant unit vectors from the float64 terms alone, R = 1 -> dC(t) = NaN"""
    ctx = blocked
    R, V = 3, 6
    vecs = synth.synth_vectors(R * F + 7, V, seed=500 + F).copy()
    vecs[:, 1] *= np.float32(1.7)                               # not unit: whole series scaled
    vecs[100:140, 2] = 0.0                                      # a few zero vectors (0/0 guard)
    vecs[:, 3] *= (1.0 + 0.2 * np.sin(np.arange(vecs.shape[0]) / 50.0)).astype(np.float32)[:, None]
    vecs[F + 5, 4] *= np.float32(1.0 + 2e-6)                    # one frame of one chunk just outside the tolerance
    Cr, dCr = c_oracle_ct(liboracle, vecs[:R * F].reshape(R, F, V, 3))
    Ct, dCt = ctx.ct_palmer(vecs, R, F)
    e = relerr(Ct, Cr)
    print('\n[ct_long kinds] F=%d: C(t) relative error %.2e per series %s' % (F, e, np.array2string(
        np.max(np.abs(Ct - Cr) / np.abs(Cr), axis=0), precision=2)))
    assert e < 1e-7 and dct_close_f32_transform(dCt, dCr, R, Cr), (F, e, np.max(np.abs(dCt - dCr)))
    const = np.zeros((2 * F, 3, 3), dtype=np.float32)
    const[:, 0, 0] = 1.0
    const[:, 1, 1] = 1.0
    const[:, 2, 2] = -1.0
    Cc, dCc = ctx.ct_palmer(const, 2, F)
    assert np.max(np.abs(Cc - 1.0)) <= 4e-15 and np.max(np.abs(dCc)) <= 4e-15
    C1, d1 = ctx.ct_palmer(vecs, 1, F)
    Cr1, _ = c_oracle_ct(liboracle, vecs[:F].reshape(1, F, V, 3))
    assert relerr(C1, Cr1) < 1e-7 and np.all(np.isnan(d1))


def test_ct_long_chunk_starts(blocked, liboracle):
    """two "files" whose first one has an odd number of frames: odd chunk starts (32-bit loads), tails dropped per file"""
    ctx = blocked
    from spinrelax_amd import ct as hostct
    F = 10000
    a = synth.synth_vectors(2 * F + 4321, 3, seed=21)
    b = synth.synth_vectors(F + 9, 3, seed=22)
    v4 = o.reformat_vecs_by_tau([a, b], 1.0, float(F))
    cat, starts, R = hostct.concat_with_chunk_starts([a, b], F)
    assert R == v4.shape[0] == 3 and starts[2] % 2 == 1
    Ct, dCt = ctx.ct_palmer(cat, R, F, chunk_start=starts)
    Cr, dCr = c_oracle_ct(liboracle, v4)
    assert relerr(Ct, Cr) < 1e-7 and dct_close_f32_transform(dCt, dCr, R, Cr)


def test_ct_long_shards_tiles_and_determinism(blocked):
    ctx = blocked
    F, R, V = 10000, 2, 6
    vecs = synth.synth_vectors(R * F, V, seed=31).copy()
    vecs[:, 2] *= np.float32(1.3)
    full, dfull = ctx.ct_palmer(vecs, R, F)
    again, dagain = ctx.ct_palmer(vecs, R, F)
    np.testing.assert_array_equal(again, full)
    np.testing.assert_array_equal(dagain, dfull)
    part, dpart = ctx.ct_palmer(vecs, R, F, v0=1, nV=3)
    np.testing.assert_array_equal(part, full[:, 1:4])
    np.testing.assert_array_equal(dpart, dfull[:, 1:4])
    # 12 series of about 0.75 MB of spectra each: a budget of 2 MiB makes tiles of two or three series, six tiles or more
    ctx.set_option('ct_long_ws_mb', 2)
    try:
        tiled, dtiled = ctx.ct_palmer(vecs, R, F)
    finally:
        ctx.set_option('ct_long_ws_mb', 256)
    np.testing.assert_array_equal(tiled, full)
    np.testing.assert_array_equal(dtiled, dfull)


def test_ct_long_agrees_with_direct_kernel(blocked):
    ctx = blocked
    F, R, V = 10000, 2, 3
    vecs = synth.synth_vectors(R * F, V, seed=41)
    Ct, dCt = ctx.ct_palmer(vecs, R, F)
    ctx.set_option('ct_fft', 0)
    try:
        Cd, dCd = ctx.ct_palmer(vecs, R, F)
    finally:
        ctx.set_option('ct_fft', 3)
    assert relerr(Ct, Cd) < 1e-7


def test_ct_long_limit(ctx):
    from spinrelax_amd.hip import SpinRelaxHipError
    assert ctx.max_frames_per_chunk() == LIMIT
    big = LIMIT + 1
    with pytest.raises(SpinRelaxHipError):
        ctx.ct_palmer(np.zeros((big, 1, 3), np.float32), 1, big)
    # the direct kernels keep their LDS limit and their error
    ctx.set_option('ct_fft', 0)
    try:
        with pytest.raises(SpinRelaxHipError):
            ctx.ct_palmer(np.zeros((20000, 1, 3), np.float32), 1, 20000)
    finally:
        ctx.set_option('ct_fft', 3)
    with pytest.raises(SpinRelaxHipError):
        ctx.ct_palmer(np.zeros((20000, 1, 3), np.float32), 1, 20000, mode=1)


def test_ct_long_pipeline_equals_staged_calls():
    """DevicePipeline on one batch at F = 10000: C(t), dC(t) and the histogram bit for bit what the stage-by-stage calls give"""
    import torch
    from spinrelax_amd import ct as hostct
    from spinrelax_amd.hip import Context
    from spinrelax_amd.pipeline import DevicePipeline
    F, R, V = 10000, 2, 8
    vecs = synth.synth_vectors(R * F, V, seed=51)
    c = Context(0)
    c.set_option('ct_long_min_frames', 5462)         # the blocked kernels at this length
    dev = torch.device('cuda', 0)
    pipe = DevicePipeline(c, dev, R * F, V, R, F, 1.0, q_rot=synth.Q_EXT, Diso=synth.DISO, aniso=synth.DANI,
                          field_MHz=(synth.FIELD_MHZ, 500.0), zeta=synth.ZETA, depth=1, stream=torch.cuda.Stream(device=dev))
    try:
        pipe.step(torch.from_numpy(vecs).to(dev))
        torch.cuda.synchronize()
        sl = pipe.slots[0]
        c.set_stream(0)
        Ct, dCt = c.ct_palmer(vecs, R, F)
        assert np.array_equal(sl.Ct.cpu().numpy(), Ct) and np.array_equal(sl.dCt.cpu().numpy(), dCt)
        e = hostct.lambert_edges()
        hist, vecsum, outer = c.rotate_hist(vecs, np.array(synth.Q_EXT), e[0], e[1], block_len=F)
        assert np.array_equal(sl.hist.cpu().numpy().reshape(hist.shape), hist)
    finally:
        pipe.close()
        c.close()
