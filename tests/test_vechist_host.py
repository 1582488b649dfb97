"""
CPU tests of kernel 2's host side (csrc/sr_vechist.hip): the range plan sr_vechist_plan, and the conditions that the inputs of
tests/test_gpu_vechist.py must meet for its comparisons to mean what they say -- computed with the float64 reference alone.
"""
import os

import numpy as np
import pytest

from conftest import ROOT                                   # noqa: F401  (puts the repository and oracle/ on sys.path)
import vechist_inputs as vi


@pytest.fixture(scope='module')
def plan():
    from spinrelax_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        from spinrelax_amd import build
        build.build(verbose=False)
    from spinrelax_amd.hip import vechist_plan
    return vechist_plan


def test_vechist_plan_invariants(plan):
    """sub is a multiple of 4 and at most 8192 (the LDS mask of a range); m ranges of sub frames cover a block and m - 1 do not; the
    ranges, by the kernel's formula, tile [0, N) exactly once and none crosses a block boundary"""
    Ns = (1, 2, 3, 4, 5, 1001, 1023, 1024, 1025, 2047, 4097, 8191, 8192, 8193, 9001, 12007, 24037, 65536, 70000)
    for N in Ns:
        for nV in (1, 7, 256, 65535):
            for bl in (0, 1, 5, 1001, 1002, 1003, 1024, 1500, N, N + 1):
                p = plan(N, nV, bl)
                what = (N, nV, bl, p)
                Fb, nB, m, sub = p['Fb'], p['nB'], p['m'], p['sub']
                assert Fb == (bl if 0 < bl <= N else N) and nB == N // Fb, what
                assert sub % 4 == 0 and 0 < sub <= 8192, what
                assert m * sub >= Fb and (m - 1) * sub < Fb, what
                start, end, in_block = vi.plan_ranges(p, N)
                assert len(start) == p['nranges'] and np.all(end > start) and np.all(end - start <= sub), what
                order = np.argsort(start, kind='stable')
                s, e = start[order], end[order]
                assert s[0] == 0 and e[-1] == N and np.array_equal(s[1:], e[:-1]), what        # every frame exactly once
                assert np.array_equal(start // Fb, (end - 1) // Fb), what                      # inside one block (or the tail)
                assert np.array_equal(in_block, end <= nB * Fb), what
    with pytest.raises(Exception):
        plan(0, 1, 0)
    with pytest.raises(Exception):
        plan(1, 0, 0)


def test_vechist_plan_of_the_gpu_cases(plan):
    """the shapes tests/test_gpu_vechist.py relies on: block starts that are 1, 2 and 3 mod 4 with several ranges per block, and a
    tail behind the last block"""
    for nV in (1, 3):
        for bl in (2047, 2049, 3001):
            p = plan(9001, nV, bl)
            start, end, in_block = vi.plan_ranges(p, 9001)
            assert p['m'] >= 2 and p['nB'] >= 2 and not in_block[-1]
            assert {int(x) for x in (np.arange(p['nB']) * bl) % 4} >= ({0, 1, 2, 3} if p['nB'] >= 4 else {0, 1})
            assert np.any(start % 4 != 0)
    for bl in (1001, 1002, 1003, 4000):
        p = plan(12007, 96, bl)
        start, end, in_block = vi.plan_ranges(p, 12007)
        assert not in_block[-1] and (np.any(start % 4 != 0) or bl % 4 == 0)
    assert np.any(vi.plan_ranges(plan(12007, 96, 1001), 12007)[0] % 4 == 1)
    assert np.any(vi.plan_ranges(plan(12007, 96, 1002), 12007)[0] % 4 == 2)
    assert np.any(vi.plan_ranges(plan(12007, 96, 1003), 12007)[0] % 4 == 3)
    p = plan(24037, 256, 1500)
    assert (p['m'], p['sub'], p['nB'], p['nranges']) == (1, 1500, 16, 17)


@pytest.mark.parametrize('name', [c[0] for c in vi.RANDOM_INPUTS])
def test_no_sample_of_a_random_input_within_1e12_of_an_edge(name):
    """device and host atan2 / acos / cos may differ in the last bits: the bit-exact comparison of counts is only meaningful when no
    sample sits that close to an edge, for every (input, quaternion, grid) the GPU tests use"""
    _, make, qs, grids = next(c for c in vi.RANDOM_INPUTS if c[0] == name)
    x = make()
    for q in qs:
        for g in grids:
            assert vi.near_edge(x, q, *g) == 0, (name, q, g)


def test_whole_sphere_input_visits_every_bin():
    h = vi.histogram(vi.rotated(vi.input_a(), None), *vi.edges(*vi.GRID))
    assert np.all(h.sum(axis=0) > 0) and h.sum() == vi.input_a().shape[0] * vi.input_a().shape[1]


def test_overflow_input_overflows_the_parked_list(plan):
    """k_vechist parks a sample whose float32 x^2 + y^2 <= 4e-3 r^2; a workgroup lists up to kListCap = 4096 parked samples and
    classifies the rest inline.  Counting only samples with x^2 + y^2 <= 3e-3 r^2 in float64 -- conservatively inside the rule --
    some workgroup of the plan holds more than 4096 of them.  With block_len = 1500 (16 blocks, m = 1) the 37-frame tail is the
    only range of the last workgroup; with block_len = 7000 (nB * m = 18) the workgroup of ranges 16 .. 19 holds two ranges of the
    last block AND two of the tail, more than 4096 parked in all.  A thread collects its mask words range by range, the tail's
    last, so it is tail samples that find the list full and take the inline path."""
    c = vi.input_c()
    per_wg, has_tail = vi.parked_per_workgroup(c, None, plan(24037, 256, 1500))
    assert np.all(per_wg[:4] > 4096) and has_tail.tolist() == [False] * 4 + [True]
    per_wg, _ = vi.parked_per_workgroup(c, vi.Q_TILT, plan(24037, 256, 1500))
    assert per_wg.max() > 4096 and per_wg.min(axis=1)[0] < 4096          # some vectors overflow, others do not
    p = plan(24037, 256, 7000)
    per_wg, has_tail = vi.parked_per_workgroup(c, None, p)
    assert np.any((per_wg.min(axis=1) > 4096) & has_tail)
    # ... and the two ranges of that workgroup that lie in a block hold fewer than 4096 frames: the overflow is the tail's
    start, end, in_block = vi.plan_ranges(p, 24037)
    wg = int(np.flatnonzero((per_wg.min(axis=1) > 4096) & has_tail)[0])
    mine = slice(4 * wg, 4 * wg + 4)
    assert in_block[mine].tolist() == [True, True, False, False] and (end[mine] - start[mine])[:2].sum() < 4096


def test_rotated_cap_is_parked_by_the_pole_rule_alone():
    """every sample of the input of test_pole_after_a_large_rotation is closer to a pole after the rotation than the kernel's rule
    admits to the float32 estimate (x^2 + y^2 <= 3e-3 r^2 in float64, conservatively inside the float32 4e-3); before the rotation
    none is: it is the rotation that brings them there"""
    x = vi.input_d2()
    for q, want in ((vi.Q_EXT, True), (None, False)):
        u = vi.rotated(x, q)
        polar = (u[..., 0] ** 2 + u[..., 1] ** 2) <= 3e-3 * (u * u).sum(axis=-1)
        assert polar.all() if want else not polar.any()
