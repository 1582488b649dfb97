"""
Inputs and the float64 reference for the tests of kernel 2 (k_vechist + k_vechist_finalize, csrc/sr_vechist.hip) on MOBILE
vectors: tests/test_vechist_host.py (the conditions on the inputs, no GPU) and tests/test_gpu_vechist.py.

synth.synth_vectors wobbles ~10 degrees about a fixed mean: a vector of 12 000 frames touches a few hundred of the 2 592 bins, never
comes near a pole and never crosses the phi = +-pi seam in bulk.  The generators here cover the sphere (iso) or sit on the poles
(cap).  They use the integer hashing of spinrelax_amd.synth and IEEE-exact float64 + - * / sqrt only, so the float32 arrays are
the same bit for bit wherever numpy runs.

Device and host atan2 / acos / cos may differ in the last bits, so a sample whose float64 phi or cos(theta) lies within 1e-12 of
a bin edge could be counted on either side.  near_edge() counts such samples; every random input of the tests has none (asserted
before the kernel is called), and no sample is ever excluded from a comparison.
"""
import numpy as np

import sr_oracle as o
from spinrelax_amd.synth import _noise, _rotate, _uniform

Q_UNNORM = (-1.3, 0.4, 2.2, -0.7)          # not normalised, negative w
Q_TILT = (0.9998, 0.02, 0.0, 0.0)          # 2.3 degrees about x: moves the poles off the z axis
Q_HALF_TURN = (0.0, 1.0, 0.0, 0.0)         # 180 degrees about x


def edges(nphi, ncos):
    """the edges np.histogramdd builds for bins=(nphi, ncos), range=((-pi, pi), (-1, 1))"""
    return np.linspace(-np.pi, np.pi, nphi + 1), np.linspace(-1.0, 1.0, ncos + 1)


def gauss(shape, seed):
    """approximately N(0, 1), one value per element (counter = its flat index).  The second term removes the exact zeros of the
    16-bit Irwin-Hall sum of _noise, which would put samples exactly on phi edges."""
    ctr = np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)
    return _noise(ctr, seed * 1000 + 21) + (_uniform(ctr, seed * 1000 + 22) - 0.5) / 37837.22761670906


def _unit_f32(g):
    return (g / np.sqrt((g * g).sum(axis=-1))[..., None]).astype(np.float32)


def iso(N, V, seed):
    """(N, V, 3) float32 directions uniform on the sphere, uncorrelated in time"""
    return _unit_f32(gauss((N, V, 3), seed))


def _cap64(N, V, seed, spread):
    g = spread * gauss((N, V, 3), seed)
    sign = np.where(np.arange(V) % 2 == 0, 1.0, -1.0)
    g[..., 2] = sign[None, :] * (1.0 + g[..., 2])
    return g


def cap(N, V, seed, spread):
    """(N, V, 3) float32 directions scattered about a pole, +z for even vectors and -z for odd ones: spread 0.02 keeps almost
    every sample within 3 degrees of it, 0.08 fills the annulus on both sides of the kernel's 3.6 degree rule"""
    return _unit_f32(_cap64(N, V, seed, spread))


def cap_seen_through(N, V, seed, spread, q):
    """cap() as it looks AFTER the rotation by q: the float64 directions are turned by the inverse of q before they are rounded to
    float32, so the kernel's rotation brings them back to the poles.  Unlike a cap that is only tilted about one axis, every
    component of the rotated vector is then a sum of terms of size 1 that cancel, and the float32 rotation of the kernel's
    estimate is off by ~5e-8 absolute: 5e-8 / sin(theta) in phi."""
    qn = np.asarray(q, dtype=np.float64)
    qn = qn / np.sqrt((qn * qn).sum())
    return _unit_f32(_rotate(qn * np.array([1.0, -1.0, -1.0, -1.0]), _cap64(N, V, seed, spread)))


def rotated(vecs, q, N=None):
    """the first N frames in float64, rotated like the reference does (q None: as they are)"""
    v = np.asarray(vecs[:N], dtype=np.float64)
    with np.errstate(invalid='ignore'):                    # NaN and infinite frames of input_g
        return v if q is None else o.rotate_vector_simd(v, np.asarray(q, dtype=np.float64))


def phi_cos(u):
    """xyz_to_rtp + cos(theta) of rotated vectors (..., 3): the two histogram coordinates, float64"""
    with np.errstate(invalid='ignore', divide='ignore'):
        rtp = o.xyz_to_rtp(u)
        return rtp[..., 1], np.cos(rtp[..., 2])


def histogram(u, edges_phi, edges_cos):
    """np.histogramdd on the given edges, per vector: (V, nphi, ncos) float64"""
    phi, c = phi_cos(u)
    out = np.empty((u.shape[1], len(edges_phi) - 1, len(edges_cos) - 1))
    for v in range(u.shape[1]):
        out[v], _ = np.histogramdd(np.stack([phi[:, v], c[:, v]], axis=-1), bins=(edges_phi, edges_cos))
    return out


_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))      # xx yy zz xy xz yz


def sums(u, block_len):
    """of rotated vectors u (N, V, 3): vecsum (V, 3) over all N frames, outer (nB, V, 6) over the full blocks of block_len frames
    (block_len outside 1 .. N: one block of N), and the sizes the error bars are made of, sum_abs (V) = sum_t |x| + |y| + |z| and
    sum_sq (nB, V) = sum_t |u|^2 per block"""
    N, V, _ = u.shape
    Fb = block_len if 0 < block_len <= N else N
    nB = N // Fb
    with np.errstate(invalid='ignore', over='ignore'):
        ub = u[: nB * Fb].reshape(nB, Fb, V, 3)
        outer = np.stack([(ub[..., i] * ub[..., j]).sum(axis=1) for i, j in _PAIRS], axis=-1)
        return dict(vecsum=u.sum(axis=0), outer=outer, sum_abs=np.abs(u).sum(axis=(0, 2)), sum_sq=(ub * ub).sum(axis=(1, 3)))


def reference(vecs, q, edges_phi, edges_cos, N, block_len):
    """what sr_rotate_hist_f32 computes, in float64 with the reference's operations: dict(hist, vecsum, outer, sum_abs, sum_sq)"""
    u = rotated(vecs, q, N)
    out = sums(u, block_len)
    out['hist'] = histogram(u, edges_phi, edges_cos)
    return out


def _edge_distance(x, lo, hi, n):
    e = np.linspace(lo, hi, n + 1)
    with np.errstate(invalid='ignore'):
        k = np.clip(np.nan_to_num(np.rint((x - lo) / (hi - lo) * n), nan=0.0, posinf=0.0, neginf=0.0), 0, n).astype(np.int64)
        return np.abs(x - e[k])


def nearest_edge(vecs, q, nphi, ncos):
    """smallest distance of a sample's float64 phi or cos(theta) from a bin edge (NaN samples do not count)"""
    phi, c = phi_cos(rotated(vecs, q))
    d = np.minimum(_edge_distance(phi, -np.pi, np.pi, nphi), _edge_distance(c, -1.0, 1.0, ncos))
    return float(np.nanmin(d))


def near_edge(vecs, q, nphi, ncos, delta=1e-12):
    """number of samples whose float64 phi or cos(theta) lies within delta of a bin edge.  A sample with a NaN coordinate (a zero
    vector: phi = 0, cos(theta) = 0 / 0) is dropped whatever the other coordinate is, and is not counted here."""
    phi, c = phi_cos(rotated(vecs, q))
    with np.errstate(invalid='ignore'):
        return int(np.count_nonzero(((_edge_distance(phi, -np.pi, np.pi, nphi) <= delta) |
                                     (_edge_distance(c, -1.0, 1.0, ncos) <= delta)) & ~np.isnan(phi) & ~np.isnan(c)))


def plan_ranges(plan, N):
    """start and end frame of every range of hip.vechist_plan's result, by the kernel's own formula (k_vechist), and whether the
    range lies in a full block: int64 arrays start, end (nranges) and bool in_block"""
    Fb, nB, m, sub, nr = plan['Fb'], plan['nB'], plan['m'], plan['sub'], plan['nranges']
    rid = np.arange(nr, dtype=np.int64)
    in_block = rid < nB * m
    b, i = rid // m, rid % m
    start = np.where(in_block, b * Fb + i * sub, nB * Fb + (rid - nB * m) * sub)
    end = np.where(in_block, np.minimum(start + sub, (b + 1) * Fb), np.minimum(start + sub, N))
    return start, end, in_block


def parked_per_workgroup(vecs, q, plan, bound=3e-3):
    """per (workgroup, vector): the number of samples the kernel is SURE to park for the pole rule -- x^2 + y^2 <= bound * r^2 in
    float64 after rotation, conservatively inside the kernel's float32 rule 4e-3 -- and per workgroup whether it holds a range
    behind the last full block.  Four ranges with consecutive numbers share a workgroup."""
    u = rotated(vecs, q)
    N = u.shape[0]
    polar = (u[..., 0] ** 2 + u[..., 1] ** 2) <= bound * (u * u).sum(axis=-1)
    cum = np.concatenate([np.zeros((1, u.shape[1]), dtype=np.int64), np.cumsum(polar, axis=0)])
    start, end, in_block = plan_ranges(plan, N)
    per_range = cum[end] - cum[start]
    nwg = (len(start) + 3) // 4
    per_wg = np.zeros((nwg, u.shape[1]), dtype=np.int64)
    np.add.at(per_wg, np.arange(len(start)) // 4, per_range)
    has_tail = np.zeros(nwg, dtype=bool)
    has_tail[np.arange(len(start))[~in_block] // 4] = True
    return per_wg, has_tail


# ---- the inputs of tests/test_gpu_vechist.py, shared with the conditions tests/test_vechist_host.py checks on them ----------------
Q_EXT = (0.866165, 0.392069, -0.308123, -0.033159)      # synth.Q_EXT
Q_NEG_W = (-0.6, 0.48, 0.0, 0.64)                       # unit, negative w
GRID = (72, 36)
GRIDS_B = ((256, 128), (1, 1), (7, 3), (36, 36), (10, 50), (90, 45))      # 256 x 128: the largest LDS grant; 90 x 45: edges by pointer
GRIDS_D = ((72, 36), (256, 128), (7, 3), (90, 45))
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
        _cache[key].setflags(write=False)
    return _cache[key]


def input_a():
    return _once('a', lambda: iso(12007, 96, 11))


def input_b():
    return _once('b', lambda: iso(12007, 8, 12))


def input_c():
    return _once('c', lambda: cap(24037, 256, 8, 0.02))


def input_d():
    return _once('d', lambda: cap(12007, 16, 9, 0.08))


def input_d2():
    """64 vectors within ~0.2 degrees of the poles AFTER the rotation by Q_EXT (cap_seen_through)"""
    return _once('d2', lambda: cap_seen_through(12007, 64, 20, 0.002, Q_EXT))


def input_e(nV):
    return _once(('e', nV), lambda: iso(9001, nV, 13 + nV))


def input_f():
    """one direction, 70 000 times: more counts in one bin than 16 bits hold"""
    d = np.array([0.3, -0.5, 0.8])
    return _once('f', lambda: np.ascontiguousarray(np.broadcast_to(_unit_f32(d), (70000, 1, 3))))


def input_g():
    """directions and values that are none: vector 0 scaled by 1e-3, 1 by 37, 2 by 1e-20 (r^2 below the kernel's 1e-30: exact path),
    a stretch of zero vectors in 3 (dropped, like numpy drops the NaN they give), three NaN frames and one infinite z in 4"""
    def make():
        v = iso(12007, 8, 17).copy()
        v[:, 0] *= np.float32(1e-3)
        v[:, 1] *= np.float32(37.0)
        v[:, 2] *= np.float32(1e-20)
        v[1000:1400, 3] = 0.0
        v[(5, 4099, 12006), 4] = np.nan
        v[7001, 4, 2] = np.inf
        return v
    return _once('g', make)


def input_h():
    return _once('h', lambda: iso(12007, 40, 16))


# (name, input, quaternions, grids) of every random input: near_edge must be 0 for each combination
RANDOM_INPUTS = (
    ('a', input_a, (None, Q_EXT, Q_UNNORM, Q_NEG_W, Q_HALF_TURN), (GRID,)),
    ('b', input_b, (Q_EXT,), GRIDS_B),
    ('c', input_c, (None, Q_TILT), (GRID,)),
    ('d', input_d, (None, Q_TILT), GRIDS_D),
    ('d2', input_d2, (Q_EXT,), (GRID, (256, 128))),
    ('e1', lambda: input_e(1), (Q_EXT,), (GRID,)),
    ('e3', lambda: input_e(3), (Q_EXT,), (GRID,)),
    ('g', input_g, (None, Q_EXT), (GRID,)),
    ('h', input_h, (Q_EXT,), (GRID,)),
)
