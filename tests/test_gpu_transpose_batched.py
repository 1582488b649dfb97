"""
GPU test of sr_transpose_batched_f64_dev (csrc/sr_ct.hip): g matrices (V, L) -> (L, V) in one launch, against torch.transpose on the
bits, with a guard behind the output.  Shapes: one element, an odd shape inside one tile, exactly 32 x 64 (whole tiles) and 33 x 65 (one
row and one column into the next tile), for one matrix and for three.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 16
NAN_BITS = 0x7ff8dead0000beef


@pytest.fixture(scope='module')
def st():
    import torch
    from spinrelax_amd.hip import Context
    ctx = Context(0)
    yield dict(torch=torch, ctx=ctx, dev=torch.device('cuda', 0))
    ctx.close()


@pytest.mark.parametrize('g', [1, 3])
@pytest.mark.parametrize('V,L', [(1, 1), (5, 33), (32, 64), (33, 65)])
def test_batched_transposition(st, g, V, L):
    torch, ctx, dev = st['torch'], st['ctx'], st['dev']
    ctx.set_stream(0)
    rng = np.random.RandomState(7 * g + V + L)
    a = torch.from_numpy(rng.standard_normal((g, V, L))).to(dev)
    a[0, 0, 0] = float('nan')                                   # bits, not values: a NaN travels like any other word
    out = torch.full((g * V * L + GUARD,), NAN_BITS, device=dev, dtype=torch.int64)
    ctx.transpose_batched_dev(a.data_ptr(), g, V, L, out.data_ptr())
    torch.cuda.synchronize()
    want = a.transpose(1, 2).contiguous().view(torch.int64).cpu().numpy()
    got = out.cpu().numpy()
    assert np.array_equal(got[:g * V * L].reshape(g, L, V), want)
    assert np.all(got[g * V * L:] == NAN_BITS)


def test_refusals(st):
    torch, ctx, dev = st['torch'], st['ctx'], st['dev']
    lib, h = ctx.lib, ctx.h
    a = torch.zeros((4,), device=dev, dtype=torch.float64)
    b = torch.full((4,), 5.0, device=dev, dtype=torch.float64)
    assert lib.sr_transpose_batched_f64_dev(h, None, 1, 2, 2, b.data_ptr()) == -2
    assert lib.sr_transpose_batched_f64_dev(h, a.data_ptr(), 1, 2, 2, None) == -2
    for g, rows, cols in ((0, 2, 2), (1, 0, 2), (1, 2, 0), (65536, 2, 2), (1, 32 * 65535 + 1, 1)):
        assert lib.sr_transpose_batched_f64_dev(h, a.data_ptr(), g, rows, cols, b.data_ptr()) == -3, (g, rows, cols)
    torch.cuda.synchronize()
    assert torch.all(b == 5.0).item()                           # nothing was queued
