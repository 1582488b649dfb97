"""
Inputs, references, the comparison and a float32 emulation for the tests of the three tile kernels of csrc/sr_noe.hip (k_noe_pairs,
k_noe_lagged, k_noe_modes: one workgroup body, csrc/sr_noe_tile.h) on MOBILE pairs: tests/test_noe_inputs_host.py (the conditions on
the inputs, the emulation against every bar and the injected errors, no GPU) and tests/test_gpu_noe_mobile.py.

make_body of tests/test_gpu_noe.py wobbles its atoms by 0.004 .. 0.025 against distances of 0.15 and more: r changes by a few percent
within a pair, the terms of every sum are nearly equal and no correlation function changes sign.  Here the nine series of
ct_dipolar_inputs.mixed (direction x distance, tests/ct_dipolar_inputs.py) become atoms.

Star layout.  Series s of a draw becomes a CENTRE c_s on a lattice (spacing 16, offset 32, 4 x 4 x n sites: exact in float32, fixed in
  time) and a SATELLITE float32(c_s + raw_s(t)).  The float32 difference satellite - centre is exact (both are multiples of the ulp of
  the smaller, 2^-19 and more, and the difference is below 2 = 2^20 such ulps), so kernel, oracle and emulation see the same d of a
  star pair.  Two
  draws (SEEDS) give P = 36 atoms and 18 star pairs (centre, own satellite) whose distance runs from 0.035 to 1.67, r^-6 within a block
  over eight orders of magnitude; the other 612 pairs are 13 and more apart and barely move: a slow control group in the same launch.
  One draw alone (P = 18, one diagonal tile) is the input of the frame-split case.
Atom order.  The canonical atoms are 2 star (centre), 2 star + 1 (satellite), star = 9 draw + series.  A layout puts them into the
  order ORDERS[name] (positions 0 .. P - 1: position / 32 is the tile) and into the columns (29 atom + 7) mod (2 P + 1) of a coordinate
  array of 2 P + 1 atoms, as test_gpu_noe_lagged.scrambled does.  With 32 atoms per tile there are three tile pairs: the diagonal tile
  0, the off-diagonal tile and the four-atom last tile.  Four atoms hold two star pairs or four satellites, never a WIDE, a CONTACT
  and the SPIKE pair in the off-diagonal AND in the last tile at once: the three layouts A, B, C together put every class into every
  tile pair (tile_classes; asserted in tests/test_noe_inputs_host.py), A is the layout of all tests, B and C those of the
  permutation test.
Quaternions.  make_body's random walk of unit quaternions (steps ~0.15 rad), independent of the coordinates: it de-tumbles nothing;
  kernel and oracle rotate d by the same R(q_t), and the lagged terms depend on it.

Every sum of the three kernels is even in d, so the reference of a layout is the reference of the canonical order with its pairs
renumbered (pair_map); tests/test_noe_inputs_host.py holds that to the oracle run on the permuted array itself.
"""
import functools

import numpy as np

import ct_dipolar_inputs as di
from spinrelax_amd import noe
from test_gpu_noe import BAR0_A3, BAR0_A6, BAR0_REFF3, BAR0_REFF6, BAR0_S2, BAR0_S2RAD, BAR0_T, oracle_derive, oracle_sums, qmul, rotmat
from test_gpu_noe import BAR1 as BAR1_MAP
from test_gpu_noe_lagged import BAR0 as BAR0_G
from test_gpu_noe_lagged import BAR1 as BAR1_G
from test_gpu_noe_lagged import BAR_LAG0, oracle_G
from test_gpu_noe_modes import BAR0 as BAR0_H
from test_gpu_noe_modes import BAR1 as BAR1_H
from test_gpu_noe_modes import BAR_IDENT, IDENT, Q_F, oracle_H

F_BLOCK = 1000
N_FRAMES = di.R * F_BLOCK + di.TAIL                  # 3016: what ct_dipolar_inputs.case_input(1000) holds
# the first draw is ct_dipolar_inputs.case_input(1000) (seed CASES[1000] = 4); the second seed is the first of 1004, 1005, ... that
# meets the conditions of tests/test_ct_dipolar_inputs_host.py at F = 1000 (asserted in tests/test_noe_inputs_host.py)
SEEDS = (di.CASES[F_BLOCK], 1006)
MIN_DIST_MOBILE = 0.03                               # what the oracles assert here: the smallest star distance is 0.0349
SPACING, OFFSET = 16.0, 32.0
TILE, STAGE, FLUSH = 32, 16, 8                       # sr_noe_tile.h: kTile, kFB, kFlush (the GPU tests assert the first two)
BLOCKS = ((0, 1000), (1000, 1000), (2000, 1000))
RAGGED = ((0, 1), (1, 499), (500, 2516))
LAGS = (0, 1, 3, 16, 17, 129, 499, 999)              # lag 999 leaves one term
LAGS_RAGGED = (0,)                                   # up to the shortest block - 1
SPLIT_BLOCK = ((0, N_FRAMES),)
SPLIT_LAGS = (0, 1, 129, 499, 1500)

SPIKE, CONTACT, WIDE, OTHER, CROSS = range(5)
CLASS_NAMES = ('spike', 'contact', 'wide', 'other star', 'cross-star')
_SERIES_CLASS = {di.FAST_SPIKE: SPIKE}
_SERIES_CLASS.update({s: CONTACT for s in di.CONTACT_SERIES})
_SERIES_CLASS.update({s: WIDE for s in di.WIDE_SERIES})


def star(draw, series):
    return di.NSER * draw + series


def centre(s):
    return 2 * s


def satellite(s):
    return 2 * s + 1


def star_class(s):
    return _SERIES_CLASS.get(s % di.NSER, OTHER)


def _order(P, tile1):
    """the canonical atoms in a scrambled order, the atoms `tile1` last (the positions 32 .. 35 of P = 36)"""
    rest = sorted((a for a in range(P) if a not in tile1), key=lambda a: (17 * a + 5) % P)
    return np.array(rest + list(tile1), dtype=np.int64)


# the four atoms of the last tile.  A: the SPIKE and a CONTACT pair off the diagonal, a WIDE pair in the last tile; B: a WIDE and the
# other SPIKE pair off the diagonal, a CONTACT pair in the last tile; C: a CONTACT and a WIDE pair off the diagonal, the SPIKE pair in it
ORDERS = {
    'A': _order(36, (satellite(star(0, di.FAST_SPIKE)), satellite(star(0, di.JUMP_CONTACT)), centre(star(0, di.FAST_WIDE)),
                     satellite(star(0, di.FAST_WIDE)))),
    'B': _order(36, (satellite(star(0, di.SLOW_WIDE)), satellite(star(1, di.FAST_SPIKE)), centre(star(0, di.WHITE_CONTACT)),
                     satellite(star(0, di.WHITE_CONTACT)))),
    'C': _order(36, (satellite(star(1, di.SHARED_CONTACT)), satellite(star(1, di.FAST_WIDE)), satellite(star(0, di.FAST_SPIKE)),
                     centre(star(0, di.FAST_SPIKE)))),
    'one': _order(18, ()),
}


def tile_classes(order):
    """{(ti, tj): set of the classes of the star pairs that tile pair computes}"""
    pos = np.argsort(order)
    out = {}
    for s in range(order.size // 2):
        a, b = sorted((int(pos[centre(s)]), int(pos[satellite(s)])))
        out.setdefault((a // TILE, b // TILE), set()).add(star_class(s))
    return out


def quat_walk(N, seed):
    """make_body's recipe: a random walk of unit quaternions, steps ~0.15 rad about random axes, w >= 0"""
    rng = np.random.default_rng(seed)
    quat = np.empty((N, 4))
    cur = np.array([1.0, 0.0, 0.0, 0.0])
    for t in range(N):
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        ang = 0.15 * rng.standard_normal()
        cur = qmul(cur, np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax]))
        cur /= np.linalg.norm(cur)
        quat[t] = cur if cur[0] >= 0 else -cur
    quat.setflags(write=False)
    return quat


@functools.lru_cache(maxsize=None)
def atoms(draws):
    """(N_FRAMES, 18 draws, 3) float32 in the canonical order, read-only"""
    out = np.empty((N_FRAMES, 2 * di.NSER * draws, 3), dtype=np.float32)
    for dr in range(draws):
        raw = di.mixed(N_FRAMES, SEEDS[dr], F_BLOCK)[2]
        for s in range(di.NSER):
            k = star(dr, s)
            c = OFFSET + SPACING * np.array([k % 4, (k // 4) % 4, k // 16], dtype=np.float64)
            out[:, centre(k)] = c
            out[:, satellite(k)] = (c[None] + raw[:, s].astype(np.float64)).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def quaternions():
    return quat_walk(N_FRAMES, 7036)


@functools.lru_cache(maxsize=None)
def layout(name):
    """(xyz (N_FRAMES, 2 P + 1, 3) float32, index (P) int32, quat (N_FRAMES, 4) float64) of ORDERS[name], read-only"""
    order = ORDERS[name]
    P = order.size
    x = atoms(P // (2 * di.NSER))
    big = np.zeros((N_FRAMES, 2 * P + 1, 3), dtype=np.float32)
    index = ((29 * order + 7) % (2 * P + 1)).astype(np.int32)
    assert np.unique(index).size == P
    big[:, index] = x[:, order]
    big.setflags(write=False)
    index.setflags(write=False)
    return big, index, quaternions()


def pair_map(order):
    """(npairs) int64: the canonical pair of every pair (i < j positions) of a layout"""
    P = order.size
    pr = noe.pair_list(P)
    a, b = order[pr[:, 0]], order[pr[:, 1]]
    return noe.pair_index(np.minimum(a, b), np.maximum(a, b), P)


def pair_classes(order):
    """(npairs) the class of every pair of a layout"""
    pr = noe.pair_list(order.size)
    a, b = order[pr[:, 0]], order[pr[:, 1]]
    is_star = (a // 2 == b // 2)
    return np.where(is_star, np.array([star_class(s) for s in a // 2]), CROSS)


def star_pairs(order):
    """(stars) int64: the pair number of every star (centre, own satellite) in a layout, by star"""
    pos = np.argsort(order)
    s = np.arange(order.size // 2)
    i, j = pos[centre(s)], pos[satellite(s)]
    return noe.pair_index(np.minimum(i, j), np.maximum(i, j), order.size)


# ---- the float64 references: the oracles of the three GPU modules on the canonical order, computed once per argument set ---------------
def _q(with_quat):
    return quaternions() if with_quat else None


@functools.lru_cache(maxsize=None)
def ref_sums(draws, with_quat, blocks):
    x = atoms(draws)
    out = oracle_sums(x, np.arange(x.shape[1]), _q(with_quat), list(blocks), min_dist=MIN_DIST_MOBILE)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_G(draws, with_quat, blocks, lags):
    x = atoms(draws)
    out = oracle_G(x, np.arange(x.shape[1]), _q(with_quat), list(blocks), list(lags), min_dist=MIN_DIST_MOBILE)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_H(draws, with_quat, with_frame, blocks, lags):
    x = atoms(draws)
    out = oracle_H(x, np.arange(x.shape[1]), _q(with_quat), Q_F if with_frame else None, list(blocks), list(lags), min_dist=MIN_DIST_MOBILE)
    for a in out:
        a.setflags(write=False)
    return out


def reference(name, blocks, lags, with_quat=True, with_frame=True, kinds=('sums', 'G', 'H')):
    """dict of the references of a layout: sums (B, npairs, 7), r3 (B, npairs); G, W (B, K, npairs); H (B, K, npairs, 6)"""
    order = ORDERS[name]
    draws, pm = order.size // (2 * di.NSER), pair_map(order)
    out = {}
    if 'sums' in kinds:
        s, r3 = ref_sums(draws, with_quat, tuple(blocks))
        out.update(sums=s[:, pm], r3=r3[:, pm])
    if 'G' in kinds:
        G, W = ref_G(draws, with_quat, tuple(blocks), tuple(lags))
        out.update(G=G[:, :, pm], W=W[:, :, pm])
    if 'H' in kinds:
        H, W = ref_H(draws, with_quat, with_frame, tuple(blocks), tuple(lags))
        out.update(H=H[:, :, pm], W=W[:, :, pm])
    return out


# ---- the comparison: measured / bar per bar and pair -----------------------------------------------------------------------------------
def ratios(got, ref, block_len, mode=0):
    """{bar name: measured / bar, one value per pair (the worst over blocks, lags and components)} of the results `got` (any of sums, G,
    H) against reference()'s dict, every bar the constant of the module that owns it: A6, T and the derived reff6, reff3, S2rad, S2, A3
    (per block and of the total) of test_gpu_noe.py, G of test_gpu_noe_lagged.py, H0 .. H5 and the identity of test_gpu_noe_modes.py,
    lag0 (G(0) against the map's own r^-6 sums)"""
    out = {}
    bl = np.asarray(block_len)
    if 'sums' in got:
        s, r = got['sums'], ref['sums']
        out['A6'] = np.max(np.abs(s[..., 0] / r[..., 0] - 1), axis=0) / (BAR1_MAP if mode else BAR0_A6)
        out['T'] = np.max(np.abs(s[..., 1:] - r[..., 1:]) / ref['r3'][..., None], axis=(0, 2)) / (BAR1_MAP if mode else BAR0_T)
        fin = noe.finalize(s, bl)
        for key, bar, rel in (('reff6', BAR0_REFF6, 1), ('reff3', BAR0_REFF3, 1), ('S2rad', BAR0_S2RAD, 1), ('S2', BAR0_S2, 0), ('A3', BAR0_A3, 1)):
            tot = oracle_derive(r.sum(axis=0), int(bl.sum()))[key]
            per = np.stack([oracle_derive(r[b], int(bl[b]))[key] for b in range(bl.size)])
            e_tot = np.abs(fin[key] / tot - 1) if rel else np.abs(fin[key] - tot)
            e_per = np.abs(fin[key + '_b'] / per - 1) if rel else np.abs(fin[key + '_b'] - per)
            out[key] = np.maximum(e_tot, e_per.max(axis=0)) / bar
    if 'G' in got:
        out['G'] = np.max(np.abs(got['G'] - ref['G']) / ref['W'], axis=(0, 1)) / (BAR1_G if mode else BAR0_G)
    if 'H' in got:
        e = np.max(np.abs(got['H'] - ref['H']) / ref['W'][..., None], axis=(0, 1))              # (npairs, 6)
        for m in range(6):
            out['H%d' % m] = e[:, m] / (BAR1_H if mode else BAR0_H[m])
    if 'G' in got and 'H' in got:
        out['ident'] = np.max(np.abs(got['H'] @ IDENT - got['G']) / ref['W'], axis=(0, 1)) / BAR_IDENT[mode]
    if 'G' in got and 'sums' in got and got.get('lags', (1,))[0] == 0:
        out['lag0'] = np.max(np.abs(got['G'][:, 0] / got['sums'][:, :, 0] - 1), axis=0) / BAR_LAG0[mode]
    return out


def worst_by_class(rat, classes):
    """{bar: (5) the largest ratio per pair class, NaN for a class without pairs}"""
    return {k: np.array([np.max(v[classes == c]) if np.any(classes == c) else np.nan for c in range(5)]) for k, v in rat.items()}


def report(tag, rat, classes):
    """prints measured / bar per bar and pair class; returns the largest ratio"""
    w = worst_by_class(rat, classes)
    print('%s: measured / bar per class (%s)' % (tag, ', '.join(CLASS_NAMES)))
    for k, v in w.items():
        print('    %-6s %s' % (k, ' '.join('%8.4f' % x for x in v)))
    return max(float(np.nanmax(v)) for v in w.values())


# ---- the split rule of sr_noe_host.h, restated ------------------------------------------------------------------------------------------
def ksplit(P, longest, B):
    nT = (P + TILE - 1) // TILE
    NP = nT * (nT + 1) // 2
    return int(min(-(-4096 // (NP * B)), max(longest // 128, 1), 256))


def lag_origins(length, k, S, s):
    no = length - k
    per = -(-no // S)
    return min(s * per, no), min(s * per + per, no)


# ---- the operation sequence of sr_noe_tile.h and of the three terms of sr_noe.hip in numpy float32 ---------------------------------------
F32, F64 = np.float32, np.float64
INJECTIONS = ('rotate_first', 'origin_matrix', 'split_shift', 'no_flush', 'ri5', 'qz_no_third')


def _fma(a, b, c):
    """one float64 product-sum (the product of two float32 is exact in float64), rounded once more to float32"""
    return (np.asarray(a, dtype=F64) * np.asarray(b, dtype=F64) + np.asarray(c, dtype=F64)).astype(F32)


def rsq_exact(x):
    """the correctly rounded reciprocal square root"""
    return (1.0 / np.sqrt(x.astype(F64))).astype(F32)


def rsq_up(x):
    """every result one float32 ulp above the correctly rounded one: with rsq_down the hardware instruction's 1-ulp tolerance"""
    return np.nextafter(rsq_exact(x), F32(np.inf))


def rsq_down(x):
    return np.nextafter(rsq_exact(x), F32(0))


def _rot(M, d):
    """d'_a = fma(Ma0, dx, fma(Ma1, dy, Ma2 dz)); M (N, 3, 3) float32 or None, d (N, n, 3)"""
    if M is None:
        return d
    return np.stack([_fma(M[:, a, 0, None], d[..., 0], _fma(M[:, a, 1, None], d[..., 1], M[:, a, 2, None] * d[..., 2])) for a in range(3)], axis=-1)


def _accumulate(items, lo, hi, no_flush):
    """float32 partial sums of FLUSH origins from lo on (a stage of 16 frames restarts them, and so does a split's first origin; 16 is
    a multiple of 8), then added in float64 in their order.  items: (a, b) per sum: acc = fma(a, b, acc), b None: acc = acc + a.
    no_flush: a last partial sum of fewer than FLUSH frames is lost.  -> (n, len(items)) float64"""
    n = items[0][0].shape[1]
    out = np.zeros((n, len(items)))
    m = hi - lo
    if m <= 0:
        return out
    g = -(-m // FLUSH)

    def groups(a):
        z = np.zeros((g * FLUSH, n), dtype=F32)
        z[:m] = a[lo:hi]
        return z.reshape(g, FLUSH, n)
    for k, (a, b) in enumerate(items):
        a8, b8 = groups(a), (None if b is None else groups(b))
        acc = np.zeros((g, n), dtype=F32)
        for f in range(FLUSH):
            acc = acc + a8[:, f] if b8 is None else _fma(a8[:, f], b8[:, f], acc)
        if no_flush and m % FLUSH:
            acc = acc[:-1]
        if acc.shape[0]:
            out[:, k] = np.cumsum(acc.astype(F64), axis=0)[-1]
    return out


def emulate_noe_f32(xyz, index, quat, frame, blocks, lags, rsq=rsq_exact, kinds=('sums', 'G', 'H'), pairs=None, inject=None):
    """What mode 0 of the three kernels computes, in numpy: dict of sums (B, n, 7), G (B, K, n), H (B, K, n, 6) (those of `kinds`) of the
    pairs `pairs` (n, 2) of positions i < j in `index` (None: all, in the library's order).  quat (N, 4) or None; frame: the frame
    quaternion of the mode sums or None (the map and the lagged map rotate by quat alone).  The split count is that of the launch
    (all of `index`).  rsq: rsq_exact, rsq_up or rsq_down.  inject: one of INJECTIONS, an error put in on purpose.  Not a bar on the
    device: what tests/test_noe_inputs_host.py uses to show that inputs and bars fit together.  Shares no code with the kernels."""
    assert inject is None or inject in INJECTIONS
    index = np.asarray(index)
    P = index.size
    pr = noe.pair_list(P) if pairs is None else np.asarray(pairs)
    x = np.ascontiguousarray(xyz[:, index], dtype=F32)
    N = x.shape[0]
    S = ksplit(P, max(n for _, n in blocks), len(blocks))
    R = None if quat is None else rotmat(np.asarray(quat, dtype=F64))
    M_map = None if R is None else R.astype(F32)
    if frame is None:
        M_modes = M_map
    else:
        Fm = rotmat(np.asarray(frame, dtype=F64)[None])[0]
        M_modes = (np.broadcast_to(Fm, (N, 3, 3)) if R is None else np.einsum('ab,tbc->tac', Fm, R)).astype(F32)

    def head(M):
        """d, ri and d' of every frame"""
        if inject == 'rotate_first' and M is not None:
            xr = _rot(M, x)
            d = xr[:, pr[:, 1]] - xr[:, pr[:, 0]]
            M = None
        else:
            d = x[:, pr[:, 1]] - x[:, pr[:, 0]]
        r2 = _fma(d[..., 2], d[..., 2], _fma(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))
        return d, rsq(r2), _rot(M, d), M

    def over_splits(items, length, k):
        tot = np.zeros((pr.shape[0], len(items)))
        for s in range(S):
            lo, hi = lag_origins(length, k, S, s)
            if inject == 'split_shift' and s >= 1:
                lo, hi = min(lo + 1, length - k), min(hi + 1, length - k)
            tot = tot + _accumulate(items, lo, hi, inject == 'no_flush')
        return tot

    out = {}
    if 'sums' in kinds:
        d, ri, p, _ = head(M_map)
        ri2 = ri * ri
        ri3 = ri2 * ri
        ri5, ri6 = ri3 * ri2, ri3 * ri3
        sx, sy, sz = p[..., 0] * ri5, p[..., 1] * ri5, p[..., 2] * ri5
        items = [(ri5 if inject == 'ri5' else ri6, None), (sx, p[..., 0]), (sy, p[..., 1]), (sz, p[..., 2]), (sx, p[..., 1]), (sx, p[..., 2]),
                 (sy, p[..., 2])]
        out['sums'] = np.stack([over_splits([(a[s0:s0 + n], None if b is None else b[s0:s0 + n]) for a, b in items], n, 0) for s0, n in blocks])
    for kind, M_kind in (('G', M_map), ('H', M_modes)):
        if kind not in kinds:
            continue
        d, ri, p, M = head(M_kind)
        res = np.empty((len(blocks), len(lags), pr.shape[0], 1 if kind == 'G' else 6))
        for b, (s0, n) in enumerate(blocks):
            for q, k in enumerate(lags):
                t0, t1 = slice(s0, s0 + n - k), slice(s0 + k, s0 + n)
                p0, p1, r0, r1 = p[t0], p[t1], ri[t0], ri[t1]
                if inject == 'origin_matrix' and M is not None:
                    p1 = _rot(M[t0], d[t1])
                g = r0 * r1
                g3 = (g * g) * g
                if kind == 'G':
                    cc = _fma(p0[..., 2], p1[..., 2], _fma(p0[..., 1], p1[..., 1], p0[..., 0] * p1[..., 0]))
                    xx = cc * g
                    items = [(_fma(F32(1.5) * xx, xx, F32(-0.5)) * g3, None)]
                else:
                    ux, uy, uz = (p0[..., a] * r0 for a in range(3))
                    vx, vy, vz = (p1[..., a] * r1 for a in range(3))
                    third = F32(0.0) if inject == 'qz_no_third' else F32(-1.0 / 3.0)
                    a0, a1 = _fma(uz, uz, third), _fma(ux, ux, -(uy * uy))
                    b0, b1 = _fma(vz, vz, third), _fma(vx, vx, -(vy * vy))
                    items = [((a0 * b0) * g3, None), ((a1 * b1) * g3, None), ((F32(0.5) * _fma(a0, b1, a1 * b0)) * g3, None),
                             (((uy * uz) * (vy * vz)) * g3, None), (((ux * uz) * (vx * vz)) * g3, None), (((ux * uy) * (vx * vy)) * g3, None)]
                res[b, q] = over_splits(items, n, k)
        out[kind] = res[..., 0] if kind == 'G' else res
    if 'G' in kinds or 'H' in kinds:
        out['lags'] = tuple(lags)
    return out


# ---- which sums one frame dominates -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shares(draws, blocks, lags):
    """the largest single-term share of sum r^-6 and of sum r^-3 (B, npairs) and of W = sum r(t)^-3 r(t + k)^-3 (B, K, npairs), in the
    canonical order"""
    x = atoms(draws).astype(np.float64)
    iu, ju = np.triu_indices(x.shape[1], k=1)
    w = ((x[:, ju] - x[:, iu]) ** 2).sum(axis=-1) ** -1.5
    s6 = np.stack([(w[s:s + n] ** 2).max(axis=0) / (w[s:s + n] ** 2).sum(axis=0) for s, n in blocks])
    s3 = np.stack([w[s:s + n].max(axis=0) / w[s:s + n].sum(axis=0) for s, n in blocks])
    sW = np.empty((len(blocks), len(lags), iu.size))
    for b, (s, n) in enumerate(blocks):
        for q, k in enumerate(lags):
            ww = w[s:s + n - k] * w[s + k:s + n]
            sW[b, q] = ww.max(axis=0) / ww.sum(axis=0)
    return s6, s3, sW
