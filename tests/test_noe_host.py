"""
CPU tests of the host side of the all-pairs dipolar map (no GPU): spinrelax_amd.noe.finalize against the literal definition, the
identities it rests on, the error convention, the pair order, select_pairs, the _noeMap.dat writer, the new entry points in the header,
the binding and the library, and the parser of scripts/calculate-Ct-from-traj.py.  The kernels: tests/test_gpu_noe.py.

Oracle (in this file): per pair and frame d = x_j - x_i in float64, r = |d|; sums of r^-6 and of d_a d_b r^-5; then
A6 = <r^-6>, A3 = <r^-3>, T = <d d^T r^-5>, S2 = 1.5 (T:T - A3^2 / 3) / A6, S2rad = A3^2 / A6 written out with plain loops over a, b.
"""
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from spinrelax_amd import _lib, noe

SCRIPT = os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')
NEW = {'sr_noe_pairs_f32_dev': 12, 'sr_noe_pairs_f32': 12, 'sr_noe_pairs_check': 9}


def frames_sums(x, blocks):
    """x (frames, P, 3) float64 -> sums (B, npairs, 7) by the definition, pairs row-major over i < j"""
    P = x.shape[1]
    iu, ju = np.triu_indices(P, k=1)
    d = x[:, ju] - x[:, iu]
    r = np.sqrt((d * d).sum(axis=-1))
    per = np.empty(d.shape[:2] + (7,))
    per[..., 0] = r ** -6
    for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        per[..., 1 + k] = d[..., a] * d[..., b] * r ** -5
    return np.stack([per[s:s + n].sum(axis=0) for s, n in blocks])


def algebra(avg):
    """averages (npairs, 7) -> A6, A3, T, reff6, reff3, S2, S2rad, element by element"""
    n = avg.shape[0]
    A6, A3, T, S2 = avg[:, 0].copy(), np.empty(n), np.empty((n, 3, 3)), np.empty(n)
    for p in range(n):
        xx, yy, zz, xy, xz, yz = avg[p, 1:]
        T[p] = [[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]
        A3[p] = xx + yy + zz
        tt = sum(T[p, a, b] ** 2 for a in range(3) for b in range(3))
        S2[p] = 1.5 * (tt - A3[p] ** 2 / 3.0) / A6[p]
    return A6, A3, T, A6 ** (-1 / 6.0), A3 ** (-1 / 3.0), S2, A3 ** 2 / A6


def body_frames(P, F, seed):
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1.0, 1.0, (P, 3)) * 1.5
    return base[None] + 0.05 * rng.standard_normal((F, P, 3))


def test_finalize_matches_the_algebra_on_random_sums():
    rng = np.random.default_rng(5)
    B, n = 3, 21
    sums = rng.uniform(0.5, 2.0, (B, n, 7))
    sums[..., 4:] -= 1.2                                       # mixed components of either sign
    bl = np.array([7, 1, 12])
    out = noe.finalize(sums, bl)
    ref = algebra(sums.sum(axis=0) / bl.sum())
    for key, r in zip(('A6', 'A3', 'T', 'reff6', 'reff3', 'S2', 'S2rad'), ref):
        assert out[key].shape == r.shape and np.max(np.abs(out[key] - r)) <= 1e-14 * np.max(np.abs(r)), key
    for b in range(B):
        refb = algebra(sums[b] / bl[b])
        for key, r in zip(('A6_b', 'A3_b', 'T_b', 'reff6_b', 'reff3_b', 'S2_b', 'S2rad_b'), refb):
            assert np.max(np.abs(out[key][b] - r)) <= 1e-14 * np.max(np.abs(r)), key
    assert out['block_len'].tolist() == [7, 1, 12]


def test_identities_on_sums_of_real_frames():
    x = body_frames(9, 40, seed=2)
    out = noe.finalize(frames_sums(x, [(0, 25), (25, 15)]), [25, 15])
    tr = out['T'][:, 0, 0] + out['T'][:, 1, 1] + out['T'][:, 2, 2]
    assert np.array_equal(tr, out['A3'])                       # the trace IS A3: the same three numbers added in the same order
    d = x[:, np.triu_indices(9, 1)[1]] - x[:, np.triu_indices(9, 1)[0]]
    A3 = (np.linalg.norm(d, axis=-1) ** -3).mean(axis=0)
    assert np.max(np.abs(out['A3'] / A3 - 1)) < 1e-13
    assert np.all(out['S2'] >= 0) and np.all(out['S2'] <= 1 + 1e-12)
    assert np.all(out['S2_b'] >= 0) and np.all(out['S2_b'] <= 1 + 1e-12)
    assert np.all(out['S2rad'] <= 1 + 1e-12) and np.all(out['S2'] <= out['S2rad'] + 1e-12)
    # a rigid pair: S2 = S2rad = 1 and both effective distances are the distance
    rigid = noe.finalize(frames_sums(np.repeat(x[:1], 5, axis=0), [(0, 5)]), [5])
    r0 = np.linalg.norm(d[0], axis=-1)
    for key, ref in (('S2', 1.0), ('S2rad', 1.0), ('reff6', r0), ('reff3', r0)):
        assert np.max(np.abs(rigid[key] - ref)) < 1e-13, key


def test_error_convention():
    x = body_frames(5, 30, seed=3)
    one = noe.finalize(frames_sums(x, [(0, 30)]), [30])
    for key in ('dS2', 'dreff6', 'dreff3'):
        assert one[key].shape == (10,) and not one[key].any(), key
    three = noe.finalize(frames_sums(x, [(0, 10), (10, 7), (17, 13)]), [10, 7, 13])
    for key, blk in (('dS2', 'S2_b'), ('dreff6', 'reff6_b'), ('dreff3', 'reff3_b')):
        ref = three[blk].std(axis=0) / (np.sqrt(3.0) - 1.0)
        assert np.max(np.abs(three[key] - ref)) <= 1e-15 and three[key].min() > 0, key
    # totals, not the mean of the block values
    assert np.max(np.abs(three['S2'] - one['S2'])) < 1e-13
    assert np.max(np.abs(three['S2_b'].mean(axis=0) - one['S2'])) > 1e-6


@pytest.mark.parametrize('P', [2, 3, 7, 32, 33, 100])
def test_pair_order_is_triu_indices(P):
    iu, ju = np.triu_indices(P, k=1)
    assert noe.n_pairs(P) == iu.size
    assert np.array_equal(noe.pair_index(iu, ju, P), np.arange(iu.size))
    assert np.array_equal(noe.pair_list(P), np.stack([iu, ju], axis=1))


def test_pair_list_at_a_size_where_the_square_root_rounds():
    P = 4099
    pl = noe.pair_list(P)
    assert pl.shape == (P * (P - 1) // 2, 2)
    assert np.array_equal(noe.pair_index(pl[:, 0], pl[:, 1], P), np.arange(pl.shape[0]))
    with pytest.raises(ValueError):
        noe.pair_index(3, 3, 10)


def test_coinciding_atoms_are_named():
    sums = frames_sums(body_frames(4, 6, seed=4), [(0, 6)])
    sums[0, noe.pair_index(1, 3, 4), 2] = np.inf
    with pytest.raises(ValueError, match=r'pair 4 \(positions 1 and 3'):
        noe.finalize(sums, [6])
    with pytest.raises(ValueError):
        noe.finalize(sums[:, :, :6], [6])
    with pytest.raises(ValueError):
        noe.finalize(sums, [6, 6])


def fake_result(P=5, seed=6):
    x = body_frames(P, 24, seed)
    res = noe.finalize(frames_sums(x, [(0, 12), (12, 12)]), [12, 12])
    res['pairs'] = noe.pair_list(P)
    res['index'] = np.array([11, 3, 29, 5, 17])[:P]
    return res


def test_select_pairs():
    res = fake_result()
    cut = float(np.sort(res['reff6'])[3])                       # the bar is inclusive: four pairs stay
    iX, iH = noe.select_pairs(res, cut)
    keep = np.nonzero(res['reff6'] <= cut)[0]
    assert keep.size == 4 and iX.dtype == np.int64 and iH.dtype == np.int64
    assert np.array_equal(iX, res['index'][res['pairs'][keep, 0]]) and np.array_equal(iH, res['index'][res['pairs'][keep, 1]])
    none = noe.select_pairs(res, 0.0)
    assert none[0].size == 0 and none[1].size == 0


def test_map_file_round_trip(tmp_path):
    res = fake_result()
    names = ['HA', 'HB2', 'HN', 'HD1', 'HG']
    fn = str(tmp_path / 'o_noeMap.dat')
    assert noe.write_map(fn, res, names=names) == 10
    with open(fn) as fp:
        assert fp.readline().split() == ['#', 'i', 'j', 'name_i', 'name_j', 'reff6', 'dreff6', 'reff3', 'S2', 'dS2', 'S2rad']
    back = noe.read_map(fn)
    assert np.array_equal(back['i'], res['index'][res['pairs'][:, 0]]) and np.array_equal(back['j'], res['index'][res['pairs'][:, 1]])
    assert back['name_i'] == [names[i] for i in res['pairs'][:, 0]] and back['name_j'] == [names[j] for j in res['pairs'][:, 1]]
    for key in ('reff6', 'dreff6', 'reff3', 'S2', 'dS2', 'S2rad'):
        assert np.max(np.abs(back[key] - res[key])) <= 5e-8 * np.max(np.abs(res[key])), key       # %.8g
    # the cutoff drops exactly the rows beyond it; the names default to the atom indices
    cut = float(np.sort(res['reff6'])[5])
    assert noe.write_map(fn, res, cutoff=cut) == 6
    back = noe.read_map(fn)
    keep = np.nonzero(res['reff6'] <= cut)[0]
    assert np.array_equal(back['i'], res['index'][res['pairs'][keep, 0]]) and back['name_i'] == [str(v) for v in back['i']]
    with pytest.raises(ValueError):
        noe.write_map(fn, res, names=['a b', 'c', 'd', 'e', 'f'])
    with pytest.raises(ValueError):
        noe.write_map(fn, res, names=['a'])


def test_library_exports_the_new_entry_points():
    if not os.path.isfile(_lib.LIB_PATH):
        from spinrelax_amd import build
        build.build(verbose=False)
    lib = _lib.load()
    for name in list(NEW) + ['sr_noe_tile', 'sr_noe_frame_batch']:
        assert hasattr(lib, name)
    assert lib.sr_noe_tile() >= 2 and lib.sr_noe_frame_batch() >= 3
    assert lib.sr_noe_pairs_f32_dev(None, None, 1, 1, None, 2, None, None, None, 1, 0, None) == -1      # no context: nothing touched
    assert lib.sr_noe_pairs_check(None, 1, 1, None, 2, None, None, 1, 0) == -1


def test_abi_declares_the_new_entry_points():
    with open(os.path.join(ROOT, 'include', 'spinrelax_hip.h')) as fp:
        text = re.sub(r'/\*.*?\*/', '', fp.read(), flags=re.S)
    for name, nargs in NEW.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        m = re.search(r'\bint %s\((.*?)\);' % name, text, flags=re.S)
        assert m and len(m.group(1).split(',')) == nargs, name
    for name in ('sr_noe_tile', 'sr_noe_frame_batch'):
        assert _lib.SIGNATURES[name][1] == [] and re.search(r'\bint %s\(void\);' % name, text), name
    assert _lib.ABI_VERSION == 13 and re.search(r'#define SR_ABI_VERSION 13\b', text)


def test_parser_accepts_the_new_flags():
    spec = importlib.util.spec_from_file_location('calc_ct_from_traj', SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.build_parser()
    a = p.parse_args(['-s', 'x.pdb', '-f', 'a.npz', '--noeMap', '--noeCutoff', '0.5'])
    assert a.bDoNoeMap is True and a.noe_cutoff == 0.5
    a = p.parse_args(['-s', 'x.pdb', '-f', 'a.npz'])
    assert a.bDoNoeMap is False and a.noe_cutoff is None
    h = p.format_help()
    assert '--noeMap' in h and '--noeCutoff' in h and h.count('[extension] all-pairs dipolar map') == 1
