"""
CPU tests (no GPU) of tests/noe_inputs.py: the conditions that make tests/test_gpu_noe_mobile.py mean something, asserted on the very
arrays the GPU tests use; the float32 emulation of the three tile kernels against every existing mode-0 bar on those arrays (the
expectation for the device, docs/EXPERIMENTS.md section 39); and six errors injected into the emulation (the teeth of the checks).

Three conditions hold differently from how they were first written down.  (1) Neither spike lies in the first block of 1000 frames (they
are the frames 1222 and 2688), and no other star pair has a frame that holds more than 0.06 of that block's sum: the blocks 1 and 2
each hold a star pair with a single-frame share above 0.8, block 0 is the block in which those pairs have no close frame.  (2) A tile
of four atoms cannot hold a WIDE, a CONTACT and the SPIKE pair: the coverage is that of the layouts A, B, C together (noe_inputs).
(3) The star pair with S2 above 0.8 has it within a block of 1000 frames (0.86, 0.87: every block's S2 is checked), 0.77 over all three.

Teeth: which injected error the checks of tests/test_gpu_noe_mobile.py (noe_inputs.ratios: every sum against its oracle, the derived
quantities, the identity, lag 0) see on the new inputs (layout A on the three blocks and the ragged table, the frame-split case) and on
make_body(33, 120) with the lags of tests/test_gpu_noe_lagged.py; the figure is the largest measured / bar, caught when above 1
(asserted in test_teeth):

    injected error                                           new inputs        make_body(33, 120)
    coordinates rotated before the difference is taken       caught (2.3e2)    caught (3.5)
    the lagged window's matrix from the origin frame         caught (2.6e5)    caught (1.3e5)
    a split's origin range shifted by one frame              caught (8.8e3)    NOT caught (0.03: one split at 120 frames)
    no flush at a stage end that is no multiple of 8         caught (1.5e5)    caught (1.9e4)
    ri5 in the place of ri6                                  caught (2.9e7)    caught (6.3e5)
    qz without the 1/3                                       caught (1.8e5)    caught (1.9e5)

The shifted split range is the one row that make_body(33, 120) misses; the frame-split cases of the existing modules (make_body(5, 300),
(33, 1000)) see it too, so no injected error is seen by the new inputs ALONE.  What the new inputs add is in the first table of
docs/EXPERIMENTS.md section 39: how much of each bar a correct kernel uses once one frame dominates a sum.
"""
import hashlib

import numpy as np
import pytest

import ct_dipolar_inputs as di
import noe_inputs as ni
from spinrelax_amd import noe
from test_gpu_noe import make_body, oracle_derive, oracle_sums
from test_gpu_noe_lagged import LAGS_120, oracle_G
from test_gpu_noe_modes import Q_F, oracle_H

SHA_300 = '9f287989d2557f48bc8d206bf424c98d93378a922c141e3db5cc3c496f6d8e71'           # layout A, frames 1000 .. 1299
# the star pairs and every 20th of the others: what the emulation is run on
EMU_CROSS_STEP = 20


def emu_pairs(order):
    cls = ni.pair_classes(order)
    keep = np.concatenate([np.nonzero(cls != ni.CROSS)[0], np.nonzero(cls == ni.CROSS)[0][::EMU_CROSS_STEP]])
    return np.sort(keep)


def test_the_inputs_are_what_the_gpu_tests_need():
    # the second seed: the first of 1004, 1005, ... that meets the conditions of test_ct_dipolar_inputs_host.py at F = 1000
    assert ni.SEEDS[0] == di.CASES[1000] == 4
    seed = 1004
    while di.failed(di.figures(1000, seed), 1000):
        seed += 1
    assert seed == ni.SEEDS[1]
    x = ni.atoms(2)
    assert x.shape == (3016, 36, 3) and x.dtype == np.float32 and not x.flags.writeable
    big, index, quat = ni.layout('A')
    assert hashlib.sha256(np.ascontiguousarray(big[1000:1300]).tobytes()).hexdigest() == SHA_300
    assert np.array_equal(big[:, index], x[:, ni.ORDERS['A']]) and np.max(np.abs((quat * quat).sum(axis=1) - 1)) < 1e-14
    # centres: exact lattice sites, fixed in time; the float32 difference of a star pair is exact
    c, s = x[:, 0::2], x[:, 1::2]
    assert np.all(c == c[0]) and np.all(c[0] % 16 == 0) and c.min() == 32.0
    d64 = s.astype(np.float64) - c.astype(np.float64)
    assert np.array_equal((s - c).astype(np.float64), d64)
    r = np.linalg.norm(d64, axis=-1)                                                   # (N, 18)
    xs = x.astype(np.float64)
    iu, ju = np.triu_indices(36, k=1)
    cross = iu // 2 != ju // 2
    rc = np.linalg.norm(xs[:, ju[cross]] - xs[:, iu[cross]], axis=-1)
    print('\n[noe inputs] star distances %.4f .. %.4f, smallest cross-star distance %.2f' % (r.min(), r.max(), rc.min()))
    assert ni.MIN_DIST_MOBILE <= r.min() < 0.036 and r.max() > 1.5 and rc.min() > 13.0
    # one frame dominates: the two spike pairs, each in its block; block 0 holds neither
    r6 = r ** -6
    share = np.stack([r6[s0:s0 + n].max(axis=0) / r6[s0:s0 + n].sum(axis=0) for s0, n in ni.BLOCKS])       # (3, 18)
    span = max((r6[s0:s0 + n].max(axis=0) / r6[s0:s0 + n].min(axis=0)).max() for s0, n in ni.BLOCKS)
    spikes = [ni.star(dr, di.FAST_SPIKE) for dr in (0, 1)]
    print('[noe inputs] largest single-frame share of sum r^-6 per block:', np.round(share.max(axis=1), 3), 'max / min of r^-6 in a block %.2g' % span)
    assert [di.spike_frame(ni.N_FRAMES, sd) // 1000 for sd in ni.SEEDS] == [1, 2]
    assert share[1, spikes[0]] >= 0.8 and share[2, spikes[1]] >= 0.8 and span > 1e8
    assert share[0].max() < 0.125 and share[0, spikes].max() < 0.01 and share[2, spikes[0]] < 0.01     # the blocks without a close frame
    assert share[:, ni.star(0, di.SLOW_CONST)].max() < 1.0011e-3
    # the oracle's C_dd changes sign inside the lag list (lab frame and with the quaternions), S2 spans 0.05 .. 0.8 in the lab frame
    sp = ni.star_pairs(np.arange(36))
    for with_quat in (False, True):
        G, W = ni.ref_G(2, with_quat, ni.BLOCKS, ni.LAGS)
        gw = (G.sum(axis=0) / W.sum(axis=0))[:, sp]
        print('[noe inputs] %s: G / W of the star pairs %.3f .. %.3f' % ('quat' if with_quat else 'lab', gw.min(), gw.max()))
        assert np.any((gw.min(axis=0) < -0.01) & (gw.max(axis=0) > 0.9))
    sums, _ = ni.ref_sums(2, False, ni.BLOCKS)
    S2 = oracle_derive(sums.sum(axis=0), 3000)['S2']
    print('[noe inputs] lab frame: S2 of the star pairs', np.round(S2[sp], 3), ' of the others %.6f .. %.6f' % (np.delete(S2, sp).min(), np.delete(S2, sp).max()))
    S2_b = np.stack([oracle_derive(sums[b], n)['S2'] for b, (_, n) in enumerate(ni.BLOCKS)])
    print('[noe inputs] lab frame: largest S2 of a star pair per block', np.round(S2_b[:, sp].max(axis=1), 3))
    assert S2[sp].min() < 0.05 and S2_b[:2, sp].max(axis=1).min() > 0.8      # above 0.8 within a block (the tests check every block), 0.77 over all
    assert S2[noe.pair_index(0, 2, 36)] > 1 - 1e-12                                      # two centres: rigid to rounding


def test_the_three_layouts_cover_every_tile_pair():
    want = {ni.SPIKE, ni.CONTACT, ni.WIDE}
    seen = {}
    for name in 'ABC':
        tc = ni.tile_classes(ni.ORDERS[name])
        assert sorted(ni.ORDERS[name]) == list(range(36)) and set(tc) == {(0, 0), (0, 1), (1, 1)}
        assert tc[(0, 0)] >= want and len(tc[(0, 1)] & want) == 2 and len(tc[(1, 1)] & want) == 1, (name, tc)
        for k, v in tc.items():
            seen.setdefault(k, set()).update(v)
    assert all(v >= want for v in seen.values()), seen
    assert sorted(ni.ORDERS['one']) == list(range(18))
    # in some star pairs the satellite comes first: d changes sign there
    pos = np.argsort(ni.ORDERS['A'])
    first = pos[0::2] < pos[1::2]
    assert first.any() and not first.all()


def test_the_renumbered_reference_is_the_oracle_on_the_permuted_array():
    """300 frames of layout B: the oracles on (xyz, index) themselves against the canonical ones renumbered by pair_map"""
    big, index, quat = ni.layout('B')
    fr = slice(1100, 1400)
    blocks, lags = [(0, 300)], [0, 7, 130]
    pm = ni.pair_map(ni.ORDERS['B'])
    x = ni.atoms(2)[fr]
    can = np.arange(36)
    a, a3 = oracle_sums(big[fr], index, quat[fr], blocks, min_dist=ni.MIN_DIST_MOBILE)
    b, b3 = oracle_sums(x, can, quat[fr], blocks, min_dist=ni.MIN_DIST_MOBILE)
    assert np.max(np.abs(a - b[:, pm]) / a3[..., None]) < 1e-14 and np.max(np.abs(a3 / b3[:, pm] - 1)) < 1e-14
    Ga, Wa = oracle_G(big[fr], index, quat[fr], blocks, lags, min_dist=ni.MIN_DIST_MOBILE)
    Gb, Wb = oracle_G(x, can, quat[fr], blocks, lags, min_dist=ni.MIN_DIST_MOBILE)
    assert np.max(np.abs(Ga - Gb[:, :, pm]) / Wa) < 1e-14
    Ha, _ = oracle_H(big[fr], index, quat[fr], Q_F, blocks, lags, min_dist=ni.MIN_DIST_MOBILE)
    Hb, _ = oracle_H(x, can, quat[fr], Q_F, blocks, lags, min_dist=ni.MIN_DIST_MOBILE)
    assert np.max(np.abs(Ha - Hb[:, :, pm]) / Wa[..., None]) < 1e-14


def test_the_split_rule_restated():
    assert (ni.ksplit(36, 1000, 3), ni.ksplit(36, 2516, 3), ni.ksplit(18, 3016, 1), ni.ksplit(33, 120, 1), ni.ksplit(5, 300, 1)) == (7, 19, 23, 1, 2)
    assert ni.lag_origins(300, 129, 2, 0) == (0, 86) and ni.lag_origins(300, 129, 2, 1) == (86, 171)      # tests/test_gpu_noe_lagged.py
    assert ni.lag_origins(1, 0, 19, 0) == (0, 1) and ni.lag_origins(1, 0, 19, 5) == (1, 1)


def emulate(name, blocks, lags, with_quat, with_frame, kinds, rsq=ni.rsq_exact, inject=None):
    big, index, quat = ni.layout(name)
    keep = emu_pairs(ni.ORDERS[name])
    got = ni.emulate_noe_f32(big, index, quat if with_quat else None, Q_F if with_frame else None, blocks, lags, rsq=rsq, kinds=kinds,
                             pairs=noe.pair_list(index.size)[keep], inject=inject)
    ref = {k: (v[:, keep] if k in ('sums', 'r3') else v[:, :, keep]) for k, v in ni.reference(name, blocks, lags, with_quat, with_frame, kinds).items()}
    return got, ref, ni.pair_classes(ni.ORDERS[name])[keep]


EMU_CASES = [('A', ni.BLOCKS, ni.LAGS, True, True, ('sums', 'G', 'H')), ('A', ni.BLOCKS, ni.LAGS, False, True, ('sums', 'G', 'H')),
             ('A', ni.RAGGED, ni.LAGS_RAGGED, True, True, ('sums', 'G', 'H')), ('one', ni.SPLIT_BLOCK, ni.SPLIT_LAGS, True, True, ('sums', 'G', 'H'))]


@pytest.mark.parametrize('rsq', (ni.rsq_exact, ni.rsq_up, ni.rsq_down), ids=('exact', 'up', 'down'))
def test_the_emulation_meets_every_mode0_bar(rsq):
    """the operation sequence in numpy float32, with the correctly rounded reciprocal square root and with every result of it one ulp up
    or down: inside every existing bar on the new inputs, whatever frame dominates.  The printed figures are the expectation for the
    device."""
    cases = EMU_CASES if rsq is ni.rsq_exact else EMU_CASES[:1]
    for name, blocks, lags, wq, wf, kinds in cases:
        got, ref, cls = emulate(name, blocks, lags, wq, wf, kinds, rsq)
        tag = '\n[emulation, rsq %s] layout %s, blocks %s, %s' % (rsq.__name__[4:], name, ' '.join('%d' % n for _, n in blocks), 'quat' if wq else 'lab')
        worst = ni.report(tag, ni.ratios(got, ref, [n for _, n in blocks]), cls)
        assert worst <= 1.0, tag


def test_the_split_case_splits_the_spike():
    """at lag 129 of the one-block case the spike frame is an origin of one split and the frame t + k of another"""
    S = ni.ksplit(18, ni.N_FRAMES, 1)
    sf = di.spike_frame(ni.N_FRAMES, ni.SEEDS[0])
    k = 129
    assert S == 23 and k in ni.SPLIT_LAGS and sf - k >= 0 and sf < ni.N_FRAMES - k

    def owner(t):
        return [s for s in range(S) if ni.lag_origins(ni.N_FRAMES, k, S, s)[0] <= t < ni.lag_origins(ni.N_FRAMES, k, S, s)[1]]
    assert len(owner(sf)) == len(owner(sf - k)) == 1 and owner(sf) != owner(sf - k)


TEETH = {'rotate_first': ('sums', 'G', 'H'), 'origin_matrix': ('G', 'H'), 'split_shift': ('sums', 'G', 'H'), 'no_flush': ('sums', 'G', 'H'),
         'ri5': ('sums',), 'qz_no_third': ('H',)}
OLD_MISSES = {'split_shift'}                       # what make_body(33, 120) cannot see: it runs in one split


def test_teeth():
    """every injected error is caught on the new inputs; on make_body(33, 120) all but the shifted split range (module docstring)"""
    _, xyz, quat = make_body(33, 120)
    index, blocks = np.arange(33), [(0, 120)]
    s, r3 = oracle_sums(xyz, index, quat, blocks)
    G, W = oracle_G(xyz, index, quat, blocks, LAGS_120)
    H, _ = oracle_H(xyz, index, quat, Q_F, blocks, LAGS_120)
    old_ref = dict(sums=s, r3=r3, G=G, H=H, W=W)
    got = ni.emulate_noe_f32(xyz, index, quat, Q_F, blocks, LAGS_120)
    assert max(v.max() for v in ni.ratios(got, old_ref, [120]).values()) <= 1.0          # without an injection: inside the bars
    print()
    for inject, kinds in TEETH.items():
        new = 0.0
        for name, bl, lags in (('A', ni.BLOCKS, ni.LAGS), ('one', ni.SPLIT_BLOCK, ni.SPLIT_LAGS)):
            g, ref, _ = emulate(name, bl, lags, True, True, kinds, inject=inject)
            new = max(new, max(np.nanmax(v) for v in ni.ratios(g, ref, [n for _, n in bl]).values()))
        g = ni.emulate_noe_f32(xyz, index, quat, Q_F, blocks, LAGS_120, kinds=kinds, inject=inject)
        with np.errstate(invalid='ignore', divide='ignore'):
            old = max(np.nanmax(v) for v in ni.ratios(g, old_ref, [120]).values())
        print('[teeth] %-14s new inputs %.2g, make_body(33, 120) %.2g' % (inject, new, old))
        assert new > 1.0, inject
        assert (old > 1.0) == (inject not in OLD_MISSES), inject
