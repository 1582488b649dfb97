"""
GPU tests of kernel 2 (k_vechist + k_vechist_finalize, csrc/sr_vechist.hip) on MOBILE vectors: every classification path of the
kernel against the float64 reference of tests/vechist_inputs.py (rotate_vector_simd, xyz_to_rtp, cos, np.histogramdd).

Counts are always compared with assert_array_equal.  tests/test_vechist_host.py shows, without a GPU, that no sample of a random
input lies within 1e-12 of a bin edge and that the inputs reach the paths they are meant for; the edge condition is asserted here
again in front of every kernel call, and no sample is ever left out of a comparison.

The bars of the float64 sums bound ANY order of summation, they are not measurements.  With u = 2^-53 and s the reference's
sum over the same frames of |x| + |y| + |z| (vecsum) or of |u|^2 (outer) of the rotated vectors:
    each vecsum component   |d| <= 4 N u s      (N - 1 additions, each within u of a partial sum that is at most s; the factor 4
                                                 covers the rotation of the sums, R s, and the reference's own rounding)
    each outer component    |d| <= 8 Fb u s     (the same over a block of Fb frames; the sums are rotated twice, R M R^T)
Every test prints its worst error / bar ratio.
"""
import numpy as np
import pytest

import vechist_inputs as vi
from spinrelax_amd._lib import SpinRelaxHipError

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope='module')
def ctx():
    from spinrelax_amd.hip import Context
    c = Context(0)
    yield c
    c.close()


_hist = {}


def ref_of(name, x, q, grid, block_len, N=None):
    """the reference of frames [0, N) of input `name`; the histogram, which does not depend on block_len, is computed once"""
    u = vi.rotated(x, q, N)
    key = (name, q, grid, N)
    if key not in _hist:
        _hist[key] = vi.histogram(u, *vi.edges(*grid))
        _hist[key].setflags(write=False)
    out = vi.sums(u, block_len)
    out['hist'] = _hist[key]
    return out


def compare(tag, got, ref, N, Fb):
    """counts bit-exact; sums within the bars wherever the reference is finite (a vector or block that holds a NaN or infinite
    frame has no bar); returns the worst error / bar ratios"""
    hist, vecsum, outer = got
    np.testing.assert_array_equal(hist, ref['hist'], err_msg=tag)
    worst = []
    for name, val, want, bar in (('vecsum', vecsum, ref['vecsum'], 4.0 * N * U * ref['sum_abs'][:, None]),
                                 ('outer', outer, ref['outer'], 8.0 * Fb * U * ref['sum_sq'][..., None])):
        assert val.shape == want.shape, (tag, name, val.shape, want.shape)
        ok = np.isfinite(want) & np.isfinite(bar)
        with np.errstate(invalid='ignore', divide='ignore'):
            err = np.where(ok, np.abs(val - want), 0.0)
            ratio = np.where(ok & (bar > 0), err / bar, 0.0)
        worst.append(float(ratio.max()))
        assert np.all(err <= np.where(ok, bar, 0.0)), (tag, name, 'worst error / bar', worst[-1])
    return worst


def run(ctx, tag, name, x, q, grid, block_len, v0=0, nV=None):
    N = x.shape[0]
    assert vi.near_edge(x, q, *grid) == 0
    cols = x if nV is None else x[:, v0:v0 + nV]
    ref = ref_of(name + (':%d+%d' % (v0, nV) if nV else ''), cols, q, grid, block_len)
    got = ctx.rotate_hist(x, q, *vi.edges(*grid), v0=v0, nV=nV, block_len=block_len)
    Fb = block_len if 0 < block_len <= N else N
    w = compare(tag, got, ref, N, Fb)
    print('%s: worst error / bar: vecsum %.3g outer %.3g' % (tag, w[0], w[1]))
    return got, ref


QS_A = {'none': None, 'q_ext': vi.Q_EXT, 'unnormalised': vi.Q_UNNORM, 'negative_w': vi.Q_NEG_W, 'half_turn': vi.Q_HALF_TURN}


@pytest.mark.parametrize('qname', list(QS_A))
def test_whole_sphere(ctx, qname):
    """a. 96 vectors uniform on the sphere, 12007 frames (odd; a tail behind the last block for every block_len but 0; block starts
    that are 1, 2, 3 mod 4 for 1001, 1002, 1003): every bin of 72 x 36 is visited, the phi seam and both poles included.  With
    the guard bands of the float32 estimate set to 0 this test fails for every quaternion (docs/EXPERIMENTS.md section 23)."""
    x = vi.input_a()
    for bl in (0, 1001, 1002, 1003, 4000):
        got, ref = run(ctx, 'a %s block_len %d' % (qname, bl), 'a', x, QS_A[qname], vi.GRID, bl)
        assert got[0].sum() == x.shape[0] * x.shape[1]
    assert np.all(ref['hist'].sum(axis=0) > 0)


@pytest.mark.parametrize('grid', vi.GRIDS_B, ids=lambda g: '%dx%d' % g)
def test_grids(ctx, grid):
    """b. 256 x 128 = 32768 bins is the largest grid (the largest LDS grant of the launch); grids that are not 2:1; one bin; 90 x 45
    has more edges than the kernel argument block holds and passes them by device pointer"""
    run(ctx, 'b %dx%d' % grid, 'b', vi.input_b(), vi.Q_EXT, grid, 1001)


def test_grids_and_shapes_refused(ctx):
    x = vi.input_b()[:64]
    with pytest.raises(SpinRelaxHipError):
        ctx.rotate_hist(x, vi.Q_EXT, *vi.edges(258, 129))                      # 33282 bins
    with pytest.raises(SpinRelaxHipError):
        ctx.rotate_hist(np.zeros((1, 65536, 3), dtype=np.float32), None, *vi.edges(*vi.GRID))


@pytest.mark.parametrize('qname,block_len', [('none', 1500), ('tilt', 1500), ('none', 7000)])
def test_parked_list_overflow(ctx, qname, block_len):
    """c. 256 vectors within ~3 degrees of a pole, 24037 frames.  block_len 1500: m = 1, a workgroup holds 4 x 1500 frames and
    parks 98 % of them, more than the 4096 its list takes, and there is a 37-frame tail (alone in the last workgroup).  With the
    poles tilted by 2.3 degrees about 69 % are parked: decided and parked samples mix, some vectors overflow and others do not.
    block_len 7000: one workgroup holds two ranges of the last block and two of the tail and overflows, so samples of a tail range
    are classified inline (tests/test_vechist_host.py::test_overflow_input_overflows_the_parked_list)."""
    q = {'none': None, 'tilt': vi.Q_TILT}[qname]
    run(ctx, 'c %s block_len %d' % (qname, block_len), 'c', vi.input_c(), q, vi.GRID, block_len)


@pytest.mark.parametrize('qname', ['none', 'tilt'])
def test_pole_annulus(ctx, qname):
    """d. 16 vectors spread ~4.6 degrees about the poles: samples on both sides of the kernel's rule x^2 + y^2 > 4e-3 r^2 (3.6
    degrees), where the float32 rotation error is amplified in phi; on four grids"""
    q = {'none': None, 'tilt': vi.Q_TILT}[qname]
    for grid in vi.GRIDS_D:
        run(ctx, 'd %s %dx%d' % ((qname,) + grid), 'd', vi.input_d(), q, grid, 1001)


@pytest.mark.parametrize('grid', [vi.GRID, (256, 128)], ids=lambda g: '%dx%d' % g)
def test_pole_after_a_large_rotation(ctx, grid):
    """d, continued.  A tilt about one axis leaves the float32 rotation of the kernel's estimate almost exact, and without a
    rotation it is exact.  Here 64 vectors lie within ~0.2 degrees of the poles only AFTER the 60 degree rotation by Q_EXT, where
    every rotated component is a sum of cancelling terms of size 1 and the estimate's phi is off by up to 4e-3 rad: every sample
    has to take the exact path, 4004 of them per workgroup (just under the 4096 of the list).  The cos(theta) guard band alone
    parks a sample within 0.27 degrees of a pole, so this input passes with and without the rule x^2 + y^2 > 4e-3 r^2
    (docs/EXPERIMENTS.md section 23 has the search for a sample that needs the rule)."""
    run(ctx, 'd2 %dx%d' % grid, 'd2', vi.input_d2(), vi.Q_EXT, grid, 1001)


@pytest.mark.parametrize('nV', [1, 3])
@pytest.mark.parametrize('block_len', [2047, 2049, 3001])
def test_unaligned_blocks_with_several_ranges(ctx, nV, block_len):
    """e. few vectors, so every block is cut into m >= 2 ranges, and block lengths that are 1 or 3 mod 4: ranges that start on a
    frame index that is no multiple of 4 (the scalar loop of vh_range) and a tail; outer is checked per block"""
    got, ref = run(ctx, 'e nV %d block_len %d' % (nV, block_len), 'e%d' % nV, vi.input_e(nV), vi.Q_EXT, vi.GRID, block_len)
    assert got[2].shape[0] == 9001 // block_len >= 2


def test_one_bin_many_counts(ctx):
    """f. 70 000 copies of one direction: one bin holds 70 000 (more than 16 bits), every other bin 0"""
    x = vi.input_f()
    for q in (None, vi.Q_EXT):
        got, ref = run(ctx, 'f %s' % (q is not None), 'f', x, q, vi.GRID, 0)
        assert got[0].max() == 70000 and np.count_nonzero(got[0]) == 1


@pytest.mark.parametrize('qname', ['none', 'q_ext'])
def test_values_that_are_not_directions(ctx, qname):
    """g. vectors scaled by 1e-3, 37 and 1e-20 (r^2 <= 1e-30: every sample takes the exact path), a stretch of zero vectors (NaN
    coordinates: dropped, like numpy drops them), three NaN frames and an infinite component in one vector.  Counts equal the
    reference; vecsum is NaN exactly where the reference's is; the sums of the other vectors meet their bars, and so do the blocks
    of the vector with the NaN frames that hold none of them."""
    x = vi.input_g()
    q = QS_A[qname]
    got, ref = run(ctx, 'g %s' % qname, 'g', x, q, vi.GRID, 1001)
    np.testing.assert_array_equal(np.isnan(got[1]), np.isnan(ref['vecsum']))
    assert np.isnan(ref['vecsum'][4]).all() and np.isfinite(ref['vecsum'][[0, 1, 2, 3, 5, 6, 7]]).all()
    per_vec = got[0].sum(axis=(1, 2))
    assert per_vec.tolist() == [12007, 12007, 12007, 12007 - 400, 12007 - 4, 12007, 12007, 12007]


@pytest.mark.parametrize('N_hist', [0, 9001, 4097])
def test_resident_path(ctx, N_hist):
    """h. the vectors appended in two parts with odd frame counts to an object that has to grow, columns 5 .. 15 of 40; the histogram
    of the first N_hist frames is bit-equal to rotate_hist on the same frames, and both match the reference"""
    x = vi.input_h()[:12006]
    e = vi.edges(*vi.GRID)
    assert vi.near_edge(x[:, 5:16], vi.Q_EXT, *vi.GRID) == 0
    with ctx.vectors(11, capacity=1000) as rv:
        rv.append(x[:5003], v0=5)
        rv.append(x[5003:], v0=5)
        assert rv.frames == 12006
        got = rv.hist(vi.Q_EXT, e[0], e[1], block_len=1001, N_hist=N_hist)
    N = N_hist or 12006
    direct = ctx.rotate_hist(x[:N], vi.Q_EXT, e[0], e[1], v0=5, nV=11, block_len=1001)
    for a, b in zip(got, direct):
        np.testing.assert_array_equal(a, b)
    ref = ref_of('h', x[:, 5:16], vi.Q_EXT, vi.GRID, 1001, N=N)
    w = compare('h %d' % N_hist, got, ref, N, 1001)
    print('h N_hist %d: worst error / bar: vecsum %.3g outer %.3g' % (N_hist, w[0], w[1]))


def test_edge_contract(ctx):
    """i. the float32 estimate of the kernel is only right for uniform edges from -pi to pi and from -1 to 1: anything else is
    refused, the numpy.linspace edges of every grid of this file are accepted"""
    x = vi.input_b()[:64]
    ephi, ecos = vi.edges(*vi.GRID)
    moved = ephi.copy()
    moved[17] += 1e-3 * (ephi[1] - ephi[0])
    moved_c = ecos.copy()
    moved_c[5] -= 1e-3 * (ecos[1] - ecos[0])
    bad = [(moved, ecos), (ephi, moved_c), (ephi[::-1].copy(), ecos), (ephi, ecos[::-1].copy()),
           (np.linspace(0.0, 2.0 * np.pi, 73), ecos), (ephi, np.linspace(0.0, 1.0, 37))]
    for ep, ec in bad:
        with pytest.raises(SpinRelaxHipError):
            ctx.rotate_hist(x, None, ep, ec)
    for grid in {vi.GRID, *vi.GRIDS_B, *vi.GRIDS_D}:
        h, _, _ = ctx.rotate_hist(x, None, *vi.edges(*grid))
        assert h.sum() == x.shape[0] * x.shape[1]


def test_run_to_run(ctx):
    """j. the overflow case twice: hist, vecsum and outer are bit-equal (integer atomics; sums combined in a fixed order)"""
    x = vi.input_c()
    e = vi.edges(*vi.GRID)
    first = ctx.rotate_hist(x, vi.Q_TILT, e[0], e[1], block_len=1500)
    second = ctx.rotate_hist(x, vi.Q_TILT, e[0], e[1], block_len=1500)
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)
