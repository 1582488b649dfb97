"""
The pure host functions of spinrelax_amd/pipeline.py: the dispatch order of the merged fit launch, the layout of the result
buffers and the cut of a run into groups.  No GPU: literals evaluated from the expressions these functions replaced.
"""
import numpy as np

from spinrelax_amd import pipeline


def test_dispatch_order_literals():
    cost = [3, 9, 3, 0, 9]
    cases = [(1, None, [0, 1, 2, 3, 4]),
             (1, cost, [1, 4, 0, 2, 3]),
             (3, None, [8, 5, 4, 14, 13, 9, 12, 11, 3, 7, 0, 2, 10, 1, 6]),
             (3, cost, [4, 14, 9, 11, 1, 6, 5, 12, 7, 0, 2, 10, 8, 13, 3])]
    for g, c, want in cases:
        p = pipeline.dispatch_order(g, 5, c)
        assert p.dtype == np.int32 and p.flags['C_CONTIGUOUS'] and p.tolist() == want, (g, c)
        p = pipeline.dispatch_order(g, 5, None if c is None else np.array(c, dtype=np.int64))
        assert p.tolist() == want, (g, c)


def test_result_layout_literals():
    dl, il = pipeline.result_layout(5, 9, 2)
    assert [e[0] for e in dl] == ['popt', 'dP', 'chisq', 'S2', 'chi', 'C', 'tau', 'relax']
    assert [e[0] for e in il] == ['status', 'nfev', 'best', 'K']
    assert pipeline.layout_cut(dl, 1)[1] == 121 and pipeline.layout_cut(il, 1)[1] == 12
    dcut, nd = pipeline.layout_cut(dl, 2)
    icut, ni = pipeline.layout_cut(il, 2)
    assert (nd, ni) == (242, 24)
    assert dcut[0] == ('popt', 0, (5, 2, 9), 1)
    assert dcut[-1] == ('relax', 210, (2, 2, 4, 2), 1)
    # every array starts where the one before it ends, and the residue axis has length n
    for cut, total in ((dcut, nd), (icut, ni)):
        o = 0
        for name, off, sh, axis in cut:
            assert off == o and sh[axis] == 2, name
            o += int(np.prod(sh))
        assert o == total
    assert {name: axis for name, _, _, axis in dcut + icut} == dict(popt=1, dP=1, chisq=1, S2=0, chi=0, C=0, tau=0, relax=1,
                                                                     status=1, nfev=1, best=0, K=0)


def test_group_sizes_literals():
    assert pipeline.group_sizes(4, 11) == [4, 4, 3]
    assert pipeline.group_sizes(4, 11, [3, 9]) == [3, 4, 4]
    assert pipeline.group_sizes(4, 0) == [] and pipeline.group_sizes(32, 5) == [5]
