"""
GPU tests of sr_ct_palmer_sums_pack_f32_dev (csrc/sr_ct.hip): the C(t) launch of one batch that carries kernel 0 of the next
(k_ct_rfft32<12, true, true>, csrc/sr_ct32.hip; the tile itself is csrc/sr_pack_tile.h, shared with k_pack_soa).

The C(t) job is F = 4096, R = 2, 32 vectors: 64 series, the cfg3 / cfg4 instantiation.  The next batch's shapes give one tile per
workgroup and two for one of them, fewer tiles than workgroups, a column offset, and more than two tiles per workgroup (the fallback:
kernel 0 in front of the C(t) kernel).  The planes must be the bytes sr_pack_soa_f32_dev writes and the sums the bits
sr_ct_palmer_sums_f32_dev gives; nothing is written behind the planes; what is refused returns its code and queues nothing.
Every case first asserts, by sr_ct_palmer_sums_pack_plan, which of the two ways the library takes.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R, F, V = 2, 4096, 32
NPAD = R * F
GUARD = 4096
NAN_PATTERN = 0x7FC00ABC


def unit_vectors(seed, N, Vtot):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((N, Vtot, 3))
    return (v / np.linalg.norm(v, axis=2, keepdims=True)).astype(np.float32)


@pytest.fixture(scope='module')
def st():
    import torch
    from spinrelax_amd.hip import Context
    ctx = Context(0)
    ctx.set_stream(0)
    dev = torch.device('cuda', 0)
    this = torch.from_numpy(unit_vectors(11, R * F, V)).to(dev)
    soa = torch.empty((V, 3, NPAD), device=dev, dtype=torch.float32)
    ctx.pack_soa_dev(this.data_ptr(), R * F, V, 0, V, soa.data_ptr(), NPAD)
    psum_len = V * R * ctx.psum_stride(F)
    want = torch.zeros(psum_len, device=dev, dtype=torch.float64)
    ctx.ct_sums_dev(soa.data_ptr(), NPAD, R, F, V, want.data_ptr())
    torch.cuda.synchronize()
    yield dict(torch=torch, ctx=ctx, dev=dev, soa=soa, want=want, psum_len=psum_len)
    ctx.close()


def guarded(st, n):
    """n floats of a NaN pattern with a guard region of the same pattern behind them"""
    torch = st['torch']
    return torch.full((n + GUARD,), NAN_PATTERN, device=st['dev'], dtype=torch.int32).view(torch.float32)


def same_bits(torch, a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_pair(st, nxt, N, Vtot, v0, nV, Npad, soa=None, F_=F, R_=R, Npad_this=NPAD, want=None, fused=None):
    """the call under test against the two separate calls: planes, sums, guard"""
    torch, ctx = st['torch'], st['ctx']
    soa = st['soa'] if soa is None else soa
    want = st['want'] if want is None else want
    n = nV * 3 * Npad
    ref = guarded(st, n)
    ctx.pack_soa_dev(nxt.data_ptr(), N, Vtot, v0, nV, ref.data_ptr(), Npad)
    got = guarded(st, n)
    psum = torch.zeros_like(want)
    args = (soa.data_ptr(), Npad_this, R_, F_, V, psum.data_ptr(), nxt.data_ptr(), N, Vtot, v0, nV, got.data_ptr(), Npad)
    if fused is not None:
        assert ctx.ct_sums_pack_plan(*args) is fused
    ctx.ct_sums_pack_dev(*args)
    torch.cuda.synchronize()
    gi, ri = got.view(torch.int32), ref.view(torch.int32)
    assert torch.equal(gi[:n], ri[:n])
    assert bool((gi[n:] == NAN_PATTERN).all()) and bool((ri[n:] == NAN_PATTERN).all())
    assert not bool(torch.isnan(got[:n]).any())
    assert torch.equal(psum.view(torch.int64), want.view(torch.int64))
    return got[:n].view(nV, 3, Npad)


@pytest.mark.parametrize('N,Npad,Vtot,v0,nV,fused', [
    (8292, 8320, 32, 0, 32, True),        # (a) 65 tiles for 64 workgroups: one packs two; N % 4 != 0, ragged last tile, zeros in [N, Npad)
    (4100, 4224, 32, 0, 32, True),        # (b) 33 tiles: fewer than workgroups
    (4100, 4224, 96, 32, 64, True),       # (c) 64 of 96 vectors from the 32nd: column offset, two tile rows
    (3 * 8292, 24896, 32, 0, 32, False),  # (d) 195 tiles > 2 x 64: kernel 0 in front of the C(t) kernel
])
def test_planes_and_sums_are_those_of_the_separate_calls(st, N, Npad, Vtot, v0, nV, fused):
    nxt = st['torch'].from_numpy(unit_vectors(N + Vtot, N, Vtot)).to(st['dev'])
    planes = run_pair(st, nxt, N, Vtot, v0, nV, Npad, fused=fused)
    host = nxt.cpu().numpy()
    got = planes.cpu().numpy()
    assert np.array_equal(got[:, :, :N], np.transpose(host[:, v0:v0 + nV], (1, 2, 0)))
    assert not got[:, :, N:].any()


def test_what_does_not_qualify_for_the_register_pack_takes_the_fallback(st):
    torch = st['torch']
    N, Npad = 4100, 4224
    flat = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), unit_vectors(5, N, 32).ravel()])).to(st['dev'])
    mis = flat[1:].view(N, 32, 3)                        # the source 4 bytes off a 16-byte boundary
    assert mis.data_ptr() % 16 == 4
    run_pair(st, mis, N, 32, 0, 32, Npad, fused=False)
    odd = torch.from_numpy(unit_vectors(6, N, 33)).to(st['dev'])        # Vtot * 3 = 99: rows are not 16-byte aligned
    run_pair(st, odd, N, 33, 0, 32, Npad, fused=False)


def test_a_chunk_length_without_a_carrying_kernel(st):
    """F = 1000 (float64 transforms by default): the same as the two separate calls"""
    torch, ctx = st['torch'], st['ctx']
    R1, F1, Np1 = 2, 1000, 2048
    this = torch.from_numpy(unit_vectors(21, R1 * F1, V)).to(st['dev'])
    soa = torch.empty((V, 3, Np1), device=st['dev'], dtype=torch.float32)
    ctx.pack_soa_dev(this.data_ptr(), R1 * F1, V, 0, V, soa.data_ptr(), Np1)
    want = torch.zeros(V * R1 * ctx.psum_stride(F1), device=st['dev'], dtype=torch.float64)
    ctx.ct_sums_dev(soa.data_ptr(), Np1, R1, F1, V, want.data_ptr())
    nxt = torch.from_numpy(unit_vectors(22, 4100, 32)).to(st['dev'])
    run_pair(st, nxt, 4100, 32, 0, 32, 4224, soa=soa, F_=F1, R_=R1, Npad_this=Np1, want=want, fused=False)


def test_refusals_queue_nothing(st):
    torch, ctx = st['torch'], st['ctx']
    call = ctx.lib.sr_ct_palmer_sums_pack_f32_dev
    N, Npad = 4100, 4224
    nxt = torch.from_numpy(unit_vectors(31, N, 32)).to(st['dev'])
    psum = torch.zeros_like(st['want'])
    dst = guarded(st, V * 3 * Npad)
    soa = st['soa']
    before = soa.clone()
    torch.cuda.synchronize()

    def rc(next_vecs, next_soa, this_soa=soa.data_ptr(), p=psum.data_ptr(), next_N=N, next_Npad=Npad):
        return call(ctx.h, this_soa, NPAD, R, F, V, None, 0, p, next_vecs, next_N, 32, 0, 32, next_soa, next_Npad)
    # the planes written are the planes read, or reach into them
    assert rc(nxt.data_ptr(), soa.data_ptr(), next_N=R * F, next_Npad=NPAD) == -3
    assert rc(nxt.data_ptr(), soa.data_ptr() + 4 * (V * 3 * NPAD - 1024)) == -3
    assert rc(nxt.data_ptr(), psum.data_ptr()) == -3
    # null pointers, of either job
    assert rc(None, dst.data_ptr()) == -2
    assert rc(nxt.data_ptr(), None) == -2
    assert rc(nxt.data_ptr(), dst.data_ptr(), this_soa=None) == -2
    assert rc(nxt.data_ptr(), dst.data_ptr(), p=None) == -2
    # the pack's own shape checks
    assert rc(nxt.data_ptr(), dst.data_ptr(), next_Npad=N - 4) == -3
    torch.cuda.synchronize()
    assert bool((dst.view(torch.int32) == NAN_PATTERN).all())
    assert same_bits(torch, soa, before) and not bool(psum.any())
