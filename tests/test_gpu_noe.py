"""
GPU tests of the all-pairs dipolar map (csrc/sr_noe.hip) and of everything above it: hip.Context.noe_pairs, spinrelax_amd.noe and the
--noeMap flag of scripts/calculate-Ct-from-traj.py.

Oracle (in this file): the literal definition in float64 numpy on the same float32 coordinates and the same float64 quaternions:
d = x_j - x_i of the coordinates converted to float64, r = |d|, d' = R(q) d, sums of r^-6 and d'_a d'_b r^-5 per block.

Inputs: a fixed body of P points on a jittered lattice (nearest neighbours 0.15 .. 0.6 apart), every point with an AR(1) wobble
(coefficient 0.9) of its own amplitude 0.004 .. 0.025, tumbled by a random walk of unit quaternions (steps ~0.15 rad), shifted 40 units
from the origin, cast to float32.  Every oracle asserts a minimum pair distance of 0.05.

Bars, u = 2^-24 (float32 unit roundoff), first order in u (the second-order terms are below 1e-5 of these).
Mode 1 (float64 throughout).  Both sides add n <= 1000 float64 terms per block, in different orders: each order is within
  (n - 1) 2^-53 sum|t| of the exact sum, the per-term arithmetic (a dozen float64 roundings) within 12 * 2^-53 |t|; together below
  2 * 1012 * 1.1e-16 = 2.3e-13 of sum|t|.  BAR1 = 1e-12: relative on the r^-6 sums (all terms positive), 1e-12 * sum r^-3 absolute
  on the tensor sums (|d'_a d'_b r^-5| <= r^-3).
Mode 0 (float32 per pair and frame), the sequence of csrc/sr_noe.hip:
  d_a = x_ja - x_ia                          u each
  r2  = fma(dz, dz, fma(dy, dy, dx dx))      2u from d, 3 roundings: 5u
  ri  = v_rsq_f32(r2)                        2.5u from r2, 1 ulp <= 2u: 4.5u
  ri2 = ri ri: 10u;  ri3 = ri2 ri: 15.5u;  ri5 = ri3 ri2: 26.5u;  ri6 = ri3 ri3: 32u
  r^-6 sums: float32 partial sums of <= 8 positive terms (7 roundings), then float64:  BAR0_A6 = 39u relative (2.3e-6);
    reff6 = A6^(-1/6): 6.5u relative.
  d'_a = fma(Ra0, dx, fma(Ra1, dy, Ra2 dz)), R rounded to float32: every product 2u from its inputs and at most 3 roundings:
    |err d'_a| <= 5u sum_b |R_ab| |d_b| <= 5u r (a row of R has unit length)
  s_a = d'_a ri5: |err| <= 5u r r^-5 + 27.5u |d'_a| r^-5 <= 32.5u r^-4
  t = s_a d'_b inside an fma: |err| <= 32.5u r^-3 + 5u r^-3 = 37.5u r^-3;  8 fma roundings of a partial sum with |sum| <= sum r^-3:
    BAR0_T = 46u * sum r^-3 absolute on the tensor sums.
  A3 = xx + yy + zz: summing the three diagonal terms first, sum_a |err t_aa| <= (10 sqrt(3) + 27.5)u r^-3 = 44.8u r^-3, and the
    three accumulations add 8u sum r^-3 together: 53u relative;  reff3: 18u relative;  S2rad = A3^2 / A6: 2 * 53u + 39u = 145u relative.
  S2 = 1.5 (T:T - A3^2 / 3) / A6 with |T|_F <= A3 (a mean of r^-3 u u^T) and |err T|_F <= 3 * 46u A3:
    |err S2| <= 1.5 (2 * 138u + 2 * 53u / 3) S2rad + 39u S2 <= 506u absolute (3.0e-5).
  A measured error above a quarter of these over >= 1000 frames would point at a systematic error; the measured worst values are in
  docs/EXPERIMENTS.md.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from spinrelax_amd import ct as hostct
from spinrelax_amd import hip, noe
from spinrelax_amd._lib import SpinRelaxHipError

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BAR1 = 1e-12
BAR0_A6, BAR0_T, BAR0_A3 = 39 * U, 46 * U, 53 * U
BAR0_REFF6, BAR0_REFF3, BAR0_S2RAD, BAR0_S2 = 6.5 * U, 18 * U, 145 * U, 506 * U
MIN_DIST = 0.05
SHIFT = 40.0


def rotmat(q):
    """(F, 4) unit quaternions (w, x, y, z) -> (F, 3, 3)"""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


@functools.lru_cache(maxsize=None)
def make_body(P, F, wobble=True, shift=SHIFT):
    """(body (P, 3) float64, xyz (F, P, 3) float32, quat (F, 4) float64): xyz[t] = R(quat[t])^T (body + wobble[t]) + shift, so that
    quat[t] takes frame t back into the body's frame.  The random numbers do not depend on `shift`."""
    rng = np.random.default_rng(7000 * P + F)
    n = int(np.ceil(P ** (1.0 / 3.0)))
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing='ij'), axis=-1).reshape(-1, 3)[:P]
    body = 0.42 * grid + rng.uniform(-0.09, 0.09, (P, 3))          # neighbours 0.42 +- 0.18 along an axis
    body -= body.mean(axis=0)
    quat = np.empty((F, 4))
    cur = np.array([1.0, 0.0, 0.0, 0.0])
    for t in range(F):
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        ang = 0.15 * rng.standard_normal()
        cur = qmul(cur, np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax]))
        cur /= np.linalg.norm(cur)
        quat[t] = cur if cur[0] >= 0 else -cur
    sig = (np.linspace(0.004, 0.025, P) if wobble else np.zeros(P))[:, None]
    w = np.empty((F, P, 3))
    x = sig * rng.standard_normal((P, 3))
    for t in range(F):
        x = 0.9 * x + np.sqrt(1 - 0.81) * sig * rng.standard_normal((P, 3))
        w[t] = x
    xyz = (np.einsum('tba,tpb->tpa', rotmat(quat), body[None] + w) + shift).astype(np.float32)
    for a in (xyz, quat, body):
        a.setflags(write=False)
    return body, xyz, quat


def oracle_sums(xyz, index, quat, blocks, min_dist=MIN_DIST):
    """sums (B, npairs, 7) and sum r^-3 (B, npairs) by the definition; asserts the minimum distance"""
    x = np.asarray(xyz[:, index], dtype=np.float64)
    iu, ju = np.triu_indices(len(index), k=1)
    d = x[:, ju] - x[:, iu]
    r = np.sqrt((d * d).sum(axis=-1))
    assert r.min() >= min_dist, 'oracle: a pair comes as close as %.3g' % r.min()
    dp = d if quat is None else np.einsum('tab,tpb->tpa', rotmat(np.asarray(quat, dtype=np.float64)), d)
    per = np.empty(d.shape[:2] + (7,))
    per[..., 0] = r ** -6
    for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        per[..., 1 + k] = dp[..., a] * dp[..., b] * r ** -5
    r3 = r ** -3
    return (np.stack([per[s:s + n].sum(axis=0) for s, n in blocks]), np.stack([r3[s:s + n].sum(axis=0) for s, n in blocks]))


def oracle_derive(sums, nframes):
    """total sums (npairs, 7) -> dict of A6, A3, reff6, reff3, S2, S2rad"""
    avg = sums / float(nframes)
    A6, A3 = avg[:, 0], avg[:, 1] + avg[:, 2] + avg[:, 3]
    TT = avg[:, 1] ** 2 + avg[:, 2] ** 2 + avg[:, 3] ** 2 + 2 * (avg[:, 4] ** 2 + avg[:, 5] ** 2 + avg[:, 6] ** 2)
    return dict(A6=A6, A3=A3, reff6=A6 ** (-1 / 6.0), reff3=A3 ** (-1 / 3.0), S2=1.5 * (TT - A3 * A3 / 3.0) / A6, S2rad=A3 * A3 / A6)


def check_sums(tag, got, ref, ref_r3, bar_a6, bar_t):
    """the two bars on raw sums; prints the measured figures before it asserts"""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    e6 = np.max(np.abs(got[..., 0] / ref[..., 0] - 1))
    et = np.max(np.abs(got[..., 1:] - ref[..., 1:]) / ref_r3[..., None])
    print('%s: r^-6 sums rel %.3g (bar %.3g), tensor sums / sum r^-3 %.3g (bar %.3g)' % (tag, e6, bar_a6, et, bar_t))
    assert e6 <= bar_a6 and et <= bar_t, tag


def check_derived(tag, res, ref):
    """the mode-0 bars on the derived quantities"""
    err = dict(reff6=np.max(np.abs(res['reff6'] / ref['reff6'] - 1)), reff3=np.max(np.abs(res['reff3'] / ref['reff3'] - 1)),
               S2rad=np.max(np.abs(res['S2rad'] / ref['S2rad'] - 1)), S2=np.max(np.abs(res['S2'] - ref['S2'])),
               A3=np.max(np.abs(res['A3'] / ref['A3'] - 1)))
    bars = dict(reff6=BAR0_REFF6, reff3=BAR0_REFF3, S2rad=BAR0_S2RAD, S2=BAR0_S2, A3=BAR0_A3)
    print('%s: ' % tag + ', '.join('%s %.3g (bar %.3g)' % (k, err[k], bars[k]) for k in sorted(err)))
    for k in err:
        assert err[k] <= bars[k], (tag, k)


@pytest.fixture(scope='module')
def ctx():
    c = hip.Context()
    yield c
    c.close()


def block_tables(F, B):
    """B = 1: all frames.  B = 3: ragged, a one-frame block first: [1, (F - 1) // 2, the rest]; with fewer than three frames one
    block per frame"""
    if B == 1:
        return [(0, F)]
    if F < 3:
        return [(t, 1) for t in range(F)]
    mid = (F - 1) // 2
    return [(0, 1), (1, mid), (1 + mid, F - 1 - mid)]


def shapes(ctx):
    T, FB = ctx.noe_tile(), ctx.noe_frame_batch()
    return [2, 3, T - 1, T, T + 1, 2 * T + 3], [1, 2, FB - 1, FB + 1, 1000]


def run_shapes(ctx, which, mode, bar_a6, bar_t):
    Ps, Fs = shapes(ctx)
    P = Ps[which]
    for F in Fs:
        _, xyz, quat = make_body(P, F)
        # the atoms in a scrambled order among twice as many: the gather by index is part of the kernel
        rng = np.random.default_rng(P + F)
        big = np.zeros((F, 2 * P + 1, 3), dtype=np.float32)
        index = rng.permutation(2 * P + 1)[:P]
        big[:, index] = xyz
        for B in (1, 3):
            blocks = block_tables(F, B)
            bs, bl = [b[0] for b in blocks], [b[1] for b in blocks]
            for q in (quat, None):
                ref, ref_r3 = oracle_sums(big, index, q, blocks)
                got = ctx.noe_pairs(big, index, quat=q, block_start=bs, block_len=bl, mode=mode)
                tag = 'mode %d P=%d F=%d B=%d %s' % (mode, P, F, len(blocks), 'quat' if q is not None else 'lab')
                check_sums(tag, got, ref, ref_r3, bar_a6, bar_t)
                if mode == 0:
                    check_derived(tag, noe.finalize(got, bl), oracle_derive(ref.sum(axis=0), sum(bl)))


@pytest.mark.parametrize('which', range(6))
def test_mode1_against_the_oracle(ctx, which):
    """P = 2, 3, T - 1, T, T + 1, 2 T + 3 (the diagonal-only tile, the first off-diagonal tile, ragged last tiles); for each
    1, 2, batch - 1, batch + 1 and 1000 frames (1000: several frame splits) as one block and as ragged blocks with a one-frame
    block, with and without quaternions.  The bar is the sum-order bound of the module docstring."""
    run_shapes(ctx, which, 1, BAR1, BAR1)


@pytest.mark.parametrize('which', range(6))
def test_mode0_against_the_oracle(ctx, which):
    """the same shapes in float32, held to the worst-case rounding bounds of the operation sequence (module docstring), on the raw
    sums and on reff6, reff3, S2rad, S2"""
    run_shapes(ctx, which, 0, BAR0_A6, BAR0_T)


def test_translation_invariance(ctx):
    """the same body at the origin and 40 units away, the oracle recomputed for each: both pass the mode-0 bars (r comes from the
    difference of the raw coordinates; a design that rotates or otherwise rounds the coordinates first fails 40 units out)"""
    P, F = ctx.noe_tile() + 1, 1000
    index = np.arange(P)
    for shift in (0.0, SHIFT):
        _, xyz, quat = make_body(P, F, True, shift)
        ref, ref_r3 = oracle_sums(xyz, index, quat, [(0, F)])
        res = noe.dipolar_map(xyz, index, quat=quat, mode=0, ctx=ctx)
        check_sums('shift %g' % shift, res['sums'], ref, ref_r3, BAR0_A6, BAR0_T)
        check_derived('shift %g' % shift, res, oracle_derive(ref[0], F))


def test_rigid_body_with_quaternions(ctx):
    """A rigid body (no wobble), tumbled: in the body's frame S2 = S2rad = 1 and reff6 = reff3 = the built distance -- up to the
    float32 rounding of the coordinates, which no kernel can undo: a coordinate below 64 is off by at most eps = 2^-19, a difference
    vector by 2 sqrt(3) eps, so distance and direction by rho = 2 sqrt(3) eps / r_min relative (4.4e-5 at r_min = 0.15); the effective
    distances are first order in rho, 1 - S2rad <= 9 rho^2 (the variance of r^-3) and 1 - S2 <= 6 rho^2 + 9 rho^2 (two directions
    2 rho apart: P2 >= 1 - 1.5 (2 rho)^2).  The oracle is held to that closed form, mode 1 with the exact quaternions as inputs to the
    oracle at 1e-12, mode 0 at its derived bars; with the front end's own quaternions (a least-squares fit to the same rounded
    coordinates, off by at most another rho) 1 - S2 <= 6 (2 rho)^2 + 9 rho^2."""
    P, F = 20, 1000
    body, xyz, quat = make_body(P, F, False)
    index = np.arange(P)
    iu, ju = np.triu_indices(P, k=1)
    built = np.linalg.norm(body[ju] - body[iu], axis=1)
    assert built.min() >= 0.15
    rho = 2 * np.sqrt(3.0) * 2.0 ** -19 / built.min()
    ref, ref_r3 = oracle_sums(xyz, index, quat, [(0, F)])
    want = oracle_derive(ref[0], F)
    for d in (want, ):
        assert np.max(np.abs(d['reff6'] / built - 1)) <= rho and np.max(np.abs(d['reff3'] / built - 1)) <= rho
        assert np.max(np.abs(d['S2rad'] - 1)) <= 9 * rho ** 2 and np.max(np.abs(d['S2'] - 1)) <= 15 * rho ** 2
    r1 = noe.dipolar_map(xyz, index, quat=quat, mode=1, ctx=ctx)
    for k in ('reff6', 'reff3', 'S2', 'S2rad'):
        e = np.max(np.abs(r1[k] / want[k] - 1))
        print('rigid, mode 1, %s: %.3g' % (k, e))
        assert e <= BAR1, k
    check_derived('rigid, mode 0', noe.dipolar_map(xyz, index, quat=quat, mode=0, ctx=ctx), want)
    # the front end's quaternions, coordinates uploaded once
    # every quantity gets the slack of its own bar
    for mode, slack in ((1, dict(S2=BAR1, S2rad=BAR1, reff6=BAR1, reff3=BAR1)),
                        (0, dict(S2=BAR0_S2, S2rad=BAR0_S2RAD, reff6=BAR0_REFF6, reff3=BAR0_REFF3))):
        rs = noe.dipolar_map_superposed(xyz, body.astype(np.float32), index, index, mode=mode, ctx=ctx)
        assert np.max(np.abs(np.abs(np.einsum('ta,ta->t', rs['quat'], quat)) - 1)) <= rho ** 2      # the same rotation, to second order
        assert np.max(np.abs(rs['S2'] - 1)) <= 33 * rho ** 2 + slack['S2']
        assert np.max(np.abs(rs['S2rad'] - 1)) <= 9 * rho ** 2 + slack['S2rad']
        assert np.max(np.abs(rs['reff6'] / built - 1)) <= rho + slack['reff6']
        assert np.max(np.abs(rs['reff3'] / built - 1)) <= rho + slack['reff3']


def test_rigid_body_without_quaternions(ctx):
    """the same tumbling body in the lab frame: S2 is the oracle's value there and far from 1 -- asserted on the oracle first"""
    P, F = 20, 1000
    _, xyz, _ = make_body(P, F, False)
    index = np.arange(P)
    ref, ref_r3 = oracle_sums(xyz, index, None, [(0, F)])
    want = oracle_derive(ref[0], F)
    assert want['S2'].max() < 0.9
    r1 = noe.dipolar_map(xyz, index, mode=1, ctx=ctx)
    # S2 from sums of mixed sign: |err T|_F <= 3 BAR1 A3 and |T|_F <= A3 give 1.5 (2 * 3 + 2 / 3) BAR1 S2rad + BAR1 S2 <= 1.2e-11
    assert np.max(np.abs(r1['S2'] - want['S2'])) <= 12 * BAR1
    assert r1['S2'].max() < 0.9
    r0 = noe.dipolar_map(xyz, index, mode=0, ctx=ctx)
    check_derived('rigid, lab frame, mode 0', r0, want)
    assert r0['S2'].max() < 0.9


def test_two_site_jump(ctx):
    """every pair alternates between two built configurations A and B with populations pA = nA / F and pB: A6 = pA rA^-6 + pB rB^-6,
    A3 likewise, T = pA dA dA^T rA^-5 + pB dB dB^T rB^-5, and S2, S2rad from them.  The coordinates are multiples of 1/64 (exact in
    float32, 40 units out too), so the closed form in float64 starts from the same numbers: 1e-12 in mode 1."""
    rng = np.random.default_rng(11)
    P, F = 6, 37
    conf = (rng.integers(-96, 97, (2, P, 3)) + 3 * 64 * np.arange(P)[None, :, None] * np.array([1, 0, 0])) / 64.0 + SHIFT
    inA = (np.arange(F) * 7) % 10 < 3
    xyz = np.where(inA[:, None, None], conf[0][None], conf[1][None]).astype(np.float32)
    assert np.array_equal(xyz.astype(np.float64), np.where(inA[:, None, None], conf[0][None], conf[1][None]))
    pA = inA.sum() / float(F)
    iu, ju = np.triu_indices(P, k=1)
    dA, dB = conf[0][ju] - conf[0][iu], conf[1][ju] - conf[1][iu]
    rA, rB = np.linalg.norm(dA, axis=1), np.linalg.norm(dB, axis=1)
    assert min(rA.min(), rB.min()) >= MIN_DIST
    A6 = pA * rA ** -6 + (1 - pA) * rB ** -6
    A3 = pA * rA ** -3 + (1 - pA) * rB ** -3
    T = pA * np.einsum('pa,pb->pab', dA, dA) * (rA ** -5)[:, None, None] + (1 - pA) * np.einsum('pa,pb->pab', dB, dB) * (rB ** -5)[:, None, None]
    S2 = 1.5 * ((T * T).sum(axis=(1, 2)) - A3 ** 2 / 3.0) / A6
    res = noe.dipolar_map(xyz, np.arange(P), blocks=([0, 20], [20, 17]), mode=1, ctx=ctx)
    for k, want in (('A6', A6), ('A3', A3), ('S2', S2), ('S2rad', A3 ** 2 / A6)):
        e = np.max(np.abs(res[k] / want - 1))
        print('two-site jump, %s: %.3g' % (k, e))
        assert e <= BAR1, k
    assert np.max(np.abs(res['T'] - T)) <= BAR1 * A3.max()


def test_agrees_with_the_dipolar_correlation_function(ctx):
    """map -> select_pairs -> ct.superpose_XHvecs -> ct.calculate_Ct_dipolar with the distances of the coordinates: reff6, reff3 and
    S2rad of the selected pairs agree to 1e-6 relative, the bar tests/test_gpu_ct_dipolar.py holds those three to"""
    P, F = 24, 1000
    body, xyz, _ = make_body(P, F)
    index = np.arange(P)
    ref32 = body.astype(np.float32)
    res = noe.dipolar_map_superposed(xyz, ref32, index, index, mode=1, ctx=ctx)      # the comparison is about the other side's float32
    iX, iH = noe.select_pairs(res, 0.6)
    assert 10 <= iX.size < noe.n_pairs(P)
    k = noe.pair_index(iX, iH, P)                                     # index = arange: atom indices are positions
    assert np.array_equal(res['pairs'][k], np.stack([iX, iH], axis=1)) and np.all(res['reff6'][k] <= 0.6)
    _, fitv = hostct.superpose_XHvecs(xyz, ref32, index, iX, iH, ctx=ctx)
    x = xyz.astype(np.float64)
    dist = np.linalg.norm(x[:, iH] - x[:, iX], axis=-1)
    R = 2
    _, _, reff6, reff3, S2rad = hostct.calculate_Ct_dipolar(fitv.reshape(R, F // R, iX.size, 3), dist=dist.reshape(R, F // R, iX.size), ctx=ctx)
    for name, a, b in (('reff6', reff6, res['reff6'][k]), ('reff3', reff3, res['reff3'][k]), ('S2rad', S2rad, res['S2rad'][k])):
        e = np.max(np.abs(a / b - 1))
        print('%s: map against calculate_Ct_dipolar %.3g' % (name, e))
        assert e <= 1e-6, name


def test_two_calls_give_the_same_bits(ctx):
    P, F = 2 * ctx.noe_tile() + 3, 1000
    _, xyz, quat = make_body(P, F)
    blocks = block_tables(F, 3)
    bs, bl = [b[0] for b in blocks], [b[1] for b in blocks]
    for mode in (0, 1):
        a = ctx.noe_pairs(xyz, np.arange(P), quat=quat, block_start=bs, block_len=bl, mode=mode)
        b = ctx.noe_pairs(xyz, np.arange(P), quat=quat, block_start=bs, block_len=bl, mode=mode)
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes()


def test_refusals_leave_the_context_usable(ctx):
    _, xyz, quat = make_body(5, 17)
    good = ctx.noe_pairs(xyz, np.arange(5), quat=quat)

    def refused(pattern, index=np.arange(5), bs=(0,), bl=(17,), mode=0, x=xyz):
        with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_noe_pairs_check: .*' + pattern):
            ctx.noe_pairs(x, index, block_start=list(bs), block_len=list(bl), mode=mode)
        again =ctx.noe_pairs(xyz, np.arange(5), quat=quat)             # the context still works, and gives the same bits
        assert again.tobytes() == good.tobytes()

    refused('a pair needs two', index=[3])
    refused(r'index\[2\] = 5 is outside the 5 atoms', index=[0, 1, 5])
    refused(r'index\[1\] = -1 is outside', index=[0, -1])
    refused(r'index\[3\] = 1 is listed twice', index=[0, 1, 2, 1])
    refused(r'block 1 = frames \[10, 18\) is outside the 17 held', bs=(0, 10), bl=(10, 8))
    refused('block 0 has length 0', bl=(0,))
    refused(r'block 0 = frames \[-1, 3\)', bs=(-1,), bl=(4,))
    refused('mode 2', mode=2)
    refused('mode -1', mode=-1)
    # a map beyond the device's memory: 40000 atoms are 8e8 pairs of 56 bytes, times 12 blocks = 537 GB
    big = np.zeros((12, 40000, 3), dtype=np.float32)
    refused('do not fit the device', index=np.arange(40000), bs=range(12), bl=[1] * 12, x=big)
    # the same through the superposed map, which allocates its sums on the device itself: the library's refusal, not an out-of-memory error
    with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_noe_pairs_check: .*do not fit the device'):
        noe.dipolar_map_superposed(big, big[0], np.arange(4), np.arange(40000), blocks=(np.arange(12), np.ones(12, dtype=np.int64)), ctx=ctx)
    assert ctx.noe_pairs(xyz, np.arange(5), quat=quat).tobytes() == good.tobytes()
    # coinciding atoms are the caller's to hear about, by name
    twice = np.array(xyz)
    twice[4, 3] = twice[4, 1]
    with pytest.raises(ValueError, match=r'pair 5 \(positions 1 and 3'):
        noe.dipolar_map(twice, np.arange(5), ctx=ctx)


def test_cli_noeMap_outputs_and_nothing_else_changes(tmp_path, ctx):
    P, F, nA = 12, 200, 20
    body, xyz, _ = make_body(nA, F)
    indexP = np.array([1, 4, 5, 7, 8, 10, 11, 13, 14, 16, 17, 19])
    names = ['H%d' % a for a in indexP]
    fit = np.arange(nA)
    ref32 = body.astype(np.float32)
    fn = str(tmp_path / 'traj.npz')
    np.savez(fn, xyz=xyz, indexX=np.array([0, 2, 3]), indexH=np.array([1, 4, 5]), ref_xyz=ref32, fit_indices=fit, indexP=indexP,
             namesP=np.array(names), dt=np.float32(10.0))
    script = os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')
    common = ['-s', 'none.pdb', '-f', fn, '--tau', '500', '--S2']
    outs = []
    for name, extra in (('plain', []), ('map', ['--noeMap', '--noeCutoff', '0.7', '--binary'])):
        d = tmp_path / name
        d.mkdir()
        p = subprocess.run([sys.executable, script] + common + ['-o', str(d / 'o')] + extra, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()[-3000:]
        outs.append(d)
    plain, withmap = (sorted(os.listdir(str(d))) for d in outs)
    assert 'o_S2.dat' in plain and sorted(plain + ['o_noeMap.dat', 'o_noeMap.npz']) == withmap      # without --noeMap no new file
    # the table against the library called directly: 4 blocks of 50 frames
    res = noe.dipolar_map_superposed(xyz, ref32, fit, indexP, blocks=([0, 50, 100, 150], [50] * 4), mode=0, ctx=ctx)
    z = np.load(str(outs[1] / 'o_noeMap.npz'))
    assert z['block_start'].tolist() == [0, 50, 100, 150] and z['block_len'].tolist() == [50] * 4
    assert z['sums'].tobytes() == res['sums'].tobytes() and np.array_equal(z['index'], indexP)
    tab = noe.read_map(str(outs[1] / 'o_noeMap.dat'))
    keep = np.nonzero(res['reff6'] <= 0.7)[0]
    assert 0 < keep.size < res['reff6'].size                                  # the cutoff drops some rows and keeps some
    assert np.array_equal(tab['i'], indexP[res['pairs'][keep, 0]]) and np.array_equal(tab['j'], indexP[res['pairs'][keep, 1]])
    assert tab['name_i'] == [names[i] for i in res['pairs'][keep, 0]] and tab['name_j'] == [names[j] for j in res['pairs'][keep, 1]]
    for key in ('reff6', 'dreff6', 'reff3', 'S2', 'dS2', 'S2rad'):
        assert np.max(np.abs(tab[key] - res[key][keep])) <= 5e-8 * np.max(np.abs(res[key][keep])), key
    assert tab['dS2'].min() > 0
