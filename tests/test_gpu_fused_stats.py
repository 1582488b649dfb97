"""
GPU tests of the model-order search fed with kernel 1's raw sums (sr_expfit_order_search_sums_f64_dev, csrc/sr_fit.hip with the
arithmetic of csrc/sr_ct_stats.h): the launch computes the chunk statistics of every residue while it stages it.  The reference is the
two-launch path of the same build -- sr_ct_finalize_t_f64_dev, then sr_expfit_order_search_batched_f64_dev -- and every comparison is on
integer views of the bits: C(t), dC(t) (residue-major) and all eleven outputs of the search, with NaN patterns in the slots of the raw
sums that nobody may read (slot 0, the slots beyond L) and guards behind every output.

Shapes, the smallest that reach every path: nRes = 2 x 3 residues; R = 1 (sd = 0 / 0), 2, 3, 24, 32 (the last count kept in registers)
and 33 (two passes over memory); F = 20, 130, 258, 600, i.e. L = 10, 65, 129, 300 -- below, at and above one point per thread for
W = 1, 2, 4 waves (64, 128, 256 threads), L > 64 W also being where the uniform-grid form of the exponentials starts; residue in LDS
and in global memory; a permuted dispatch order on the fused side only (results stay at the residue's index); one or nRes rows of
tau guesses; orders (2, 3, 5, 7, 9) and one run with 11.
"""
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NB, V = 2, 3
NRES = NB * V
ORDERS = (2, 3, 5, 7, 9)
GUARD = 16
RS = (1, 2, 3, 24, 32, 33)
NAN_BITS = 0x7ff8dead0000beef            # the pattern of the slots nobody reads and of the float64 guards
INT_GUARD = -1234567
DT = 10.0


@pytest.fixture(scope='module')
def st():
    import torch
    from spinrelax_amd.hip import Context
    ctx = Context(0)
    yield dict(torch=torch, ctx=ctx, dev=torch.device('cuda', 0), sums={})
    ctx.set_option('fit_waves', 2)
    ctx.set_option('fit_lds', 1)
    ctx.close()


def host_sums(st, R, F):
    """(NRES, R, Lp) raw sums of a decaying C(t) plus per-chunk noise, S = (C + 0.5) / 1.5 (F - d), so that the fits converge;
    NaN pattern in slot 0 and beyond L.  Made once per shape and left unchanged."""
    if (R, F) in st['sums']:
        return st['sums'][R, F]
    L, Lp = F // 2, st['ctx'].psum_stride(F)
    rng = np.random.RandomState(1000 * R + F)
    t = (np.arange(L) + 1.0) * DT
    S2 = np.linspace(0.55, 0.85, NRES)[:, None]
    tau = np.geomspace(3.0 * DT, 0.4 * L * DT, NRES)[:, None]
    C = S2 + (1.0 - S2) * np.exp(-t[None, :] / tau)                              # (NRES, L)
    Cr = C[:, None, :] + 2e-3 * rng.standard_normal((NRES, R, L))               # per chunk
    sums = np.empty((NRES, R, Lp), dtype=np.float64)
    sums.view(np.int64)[...] = NAN_BITS
    sums[:, :, 1:L + 1] = (Cr + 0.5) / 1.5 * (F - np.arange(1, L + 1))
    st['sums'][R, F] = sums
    return sums


class Outputs:
    """CtT, dCtT and the eleven result arrays of a search over NRES residues, each with a guard behind it"""
    F64 = ('CtT', 'dCtT', 'popt', 'dP', 'chisq', 'S2', 'C', 'tau', 'chi')
    I32 = ('status', 'nfev', 'best', 'K')

    def __init__(self, st, L, orders):
        torch, dev = st['torch'], st['dev']
        nO, Pmax = len(orders), max(orders)
        Kmax = Pmax // 2
        self.n = dict(CtT=NRES * L, dCtT=NRES * L, popt=nO * NRES * Pmax, dP=nO * NRES * Pmax, chisq=nO * NRES, S2=NRES, C=NRES * Kmax,
                      tau=NRES * Kmax, chi=NRES, status=nO * NRES, nfev=nO * NRES, best=NRES, K=NRES)
        self.t = {}
        for name in self.F64:
            self.t[name] = torch.full((self.n[name] + GUARD,), NAN_BITS, device=dev, dtype=torch.int64).view(torch.float64)
        for name in self.I32:
            self.t[name] = torch.full((self.n[name] + GUARD,), INT_GUARD, device=dev, dtype=torch.int32)

    def ptr(self, name):
        return self.t[name].data_ptr()

    def results(self):
        return [self.ptr(n) for n in ('popt', 'dP', 'chisq', 'status', 'nfev', 'best', 'S2', 'C', 'tau', 'chi', 'K')]

    def host(self):
        """{name: (bits of the array, bits of its guard)}"""
        out = {}
        for name, tns in self.t.items():
            a = tns.cpu().numpy()
            a = a.view(np.int64) if a.dtype == np.float64 else a
            out[name] = (a[:self.n[name]].copy(), a[self.n[name]:].copy())
        return out


def both_ways(st, R, F, W, lds, orders=ORDERS, tau_rows=1, permute=True):
    """the two-launch path and the fused launch on the same raw sums: ({name: (bits, guard bits)} of each, the raw sums)"""
    from spinrelax_amd import fitting_Ct_functions as fitCt
    torch, ctx, dev = st['torch'], st['ctx'], st['dev']
    L = F // 2
    ctx.set_stream(0)
    ctx.set_option('fit_waves', W)
    ctx.set_option('fit_lds', lds)
    sums_h = host_sums(st, R, F)
    sums = torch.from_numpy(sums_h).to(dev)
    t_h = (np.arange(L) + 1.0) * DT
    t = torch.from_numpy(t_h).to(dev)
    tg = fitCt.tau_guesses(t_h, orders)                                          # (1, sum K)
    if tau_rows != 1:
        tg = np.ascontiguousarray(tg * (1.0 + 0.01 * np.arange(NRES))[:, None])  # a row of its own per residue
    tg_d = torch.from_numpy(np.ascontiguousarray(tg)).to(dev)
    tau_max = 10.0 * t_h[-1]
    work = torch.empty((NRES * L,), device=dev, dtype=torch.float64)
    order = torch.tensor([4, 0, 5, 2, 1, 3], device=dev, dtype=torch.int32) if permute else None
    # reference: the chunk statistics of each batch of V series, then the search on their output, natural order
    ref = Outputs(st, L, orders)
    Ct = torch.empty((NB, L, V), device=dev, dtype=torch.float64)
    dCt = torch.empty_like(Ct)
    for b in range(NB):
        ctx.ct_finalize_dev(sums[b * V:].data_ptr(), R, F, V, Ct[b].data_ptr(), dCt[b].data_ptr(),
                            ref.ptr('CtT') + b * V * L * 8, ref.ptr('dCtT') + b * V * L * 8)
    ctx.order_search_batched_dev(t.data_ptr(), 1, ref.ptr('CtT'), ref.ptr('dCtT'), NRES, L, orders, tg_d.data_ptr(), tau_rows, tau_max, 0.5,
                                 *ref.results(), work_ptr=work.data_ptr())
    torch.cuda.synchronize()
    # fused
    got = Outputs(st, L, orders)
    ctx.order_search_sums_dev(t.data_ptr(), 1, sums.data_ptr(), R, F, got.ptr('CtT'), got.ptr('dCtT'), NRES, L, orders, tg_d.data_ptr(),
                              tau_rows, tau_max, 0.5, *got.results(), work_ptr=work.data_ptr(),
                              dispatch_order_ptr=None if order is None else order.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(sums.cpu().numpy().view(np.int64), sums_h.view(np.int64))          # the raw sums are only read
    return ref.host(), got.host(), (Ct.cpu().numpy(), dCt.cpu().numpy())


def assert_same(ref, got, what):
    assert set(ref) == set(Outputs.F64 + Outputs.I32)
    for name in ref:
        a, ga = ref[name]
        b, gb = got[name]
        print('%s %s: %d of %d words differ' % (what, name, int((a != b).sum()), a.size))
        assert np.array_equal(a, b), (what, name)
        pattern = NAN_BITS if name in Outputs.F64 else INT_GUARD
        assert np.all(ga == pattern) and np.all(gb == pattern), (what, name, 'guard')


@pytest.mark.parametrize('F', [20, 130, 258, 600])
@pytest.mark.parametrize('W,lds', [(1, 1), (2, 1), (4, 1), (1, 0), (2, 0), (4, 0)])
def test_fused_staging_gives_the_bits_of_the_two_launch_path(st, W, lds, F):
    L = F // 2
    for i, R in enumerate(RS):
        ref, got, (Ct, dCt) = both_ways(st, R, F, W, lds, tau_rows=1 if i % 2 == 0 else NRES)
        assert_same(ref, got, 'R=%d F=%d W=%d lds=%d' % (R, F, W, lds))
        CtT = got['CtT'][0].view(np.float64).reshape(NB, V, L)
        dCtT = got['dCtT'][0].view(np.float64).reshape(NB, V, L)
        # the reference really is what k_ct_finalize leaves in both orientations, and the data are what they were built to be
        assert np.array_equal(CtT.transpose(0, 2, 1), Ct) and np.array_equal(dCtT.transpose(0, 2, 1), dCt, equal_nan=True)
        assert np.all(np.isfinite(CtT)) and np.all(CtT > 0.4) and np.all(CtT < 1.1)
        status = got['status'][0].reshape(len(ORDERS), NRES)
        assert np.all(status[0] != -100)                                         # every residue's search ran
        if R == 1:
            assert np.all(np.isnan(dCtT))                                        # 0 / 0, as the reference code gives it
        else:
            assert np.all(dCtT > 0) and np.all(dCtT < 0.05)
            nfev = got['nfev'][0].reshape(len(ORDERS), NRES)
            print('R=%d F=%d W=%d lds=%d: %d of %d residues selected a model, %d evaluations' % (R, F, W, lds, int((got['best'][0] >= 0).sum()), NRES, int(nfev.sum())))
            assert np.all(nfev[0] > 0)


def test_order_eleven(st):
    ref, got, _ = both_ways(st, 3, 258, 2, 1, orders=(2, 3, 5, 7, 9, 11))
    assert_same(ref, got, 'order 11')
    assert np.all(got['status'][0].reshape(6, NRES)[0] != -100)


def test_natural_dispatch_order(st):
    ref, got, _ = both_ways(st, 24, 130, 2, 1, permute=False)
    assert_same(ref, got, 'natural order')


def test_contraction_matters_in_the_input(st):
    """k_ct_finalize computes 1.5 q - 0.5 as ONE fused multiply-add; a staging that rounded the product first would differ in the last
    bit for inputs like these -- counted here on the host, in exact arithmetic, for the sums of a case the comparison above runs"""
    R, F = 3, 130
    L = F // 2
    sums = host_sums(st, R, F)
    n = (F - np.arange(1, L + 1)).astype(np.float64)
    q = sums[:, :, 1:L + 1] / n                                                  # IEEE division, as on the device
    unfused = 1.5 * q - 0.5                                                      # two roundings
    fused = np.array([float(Fraction(1.5) * Fraction(float(x)) - Fraction(1, 2)) for x in q.ravel()]).reshape(q.shape)   # one
    differ = int((unfused.view(np.int64) != fused.view(np.int64)).sum())
    print('1.5 q - 0.5: %d of %d values differ between the fused and the unfused form' % (differ, q.size))
    # (few: S was made from C by the inverse operations, so 1.5 q mostly lands next to a double; what counts is that there are some)
    assert differ > 0
    assert np.all(np.abs(unfused - fused) <= np.spacing(np.abs(fused)))          # ... and by one unit in the last place
    ref, got, _ = both_ways(st, R, F, 2, 1)
    assert_same(ref, got, 'contraction')
    # the device's C(t) is the mean of the FUSED values
    m = (fused[:, 0] + fused[:, 1] + fused[:, 2]) / 3.0
    m_unfused = (unfused[:, 0] + unfused[:, 1] + unfused[:, 2]) / 3.0
    CtT = got['CtT'][0].view(np.float64).reshape(NRES, L)
    assert np.array_equal(CtT, m) and not np.array_equal(CtT, m_unfused)        # ... and the unfused form would have shown


def test_refusals(st):
    torch, ctx, dev = st['torch'], st['ctx'], st['dev']
    lib, h = ctx.lib, ctx.h
    R, F = 3, 20
    L = F // 2
    sums = torch.from_numpy(host_sums(st, R, F)).to(dev)
    o = Outputs(st, L, ORDERS)
    t = torch.arange(1, L + 1, device=dev, dtype=torch.float64)
    orders = np.ascontiguousarray(ORDERS, dtype=np.int32)
    tg = torch.ones((13,), device=dev, dtype=torch.float64)

    def call(sums_ptr=sums.data_ptr(), R=R, F=F, CtT=o.ptr('CtT'), dCtT=o.ptr('dCtT'), L=L):
        return lib.sr_expfit_order_search_sums_f64_dev(h, t.data_ptr(), 1, sums_ptr, R, F, CtT, dCtT, NRES, L, orders.ctypes.data, len(ORDERS),
                                                       tg.data_ptr(), 1, 1000.0, 0.5, None, None, 0, None, *o.results())
    assert call(sums_ptr=None) == -2 and call(CtT=None) == -2 and call(dCtT=None) == -2
    assert call(R=0) == -3 and call(F=1, L=0) == -3 and call(L=L - 1) == -3 and call(F=F + 2) == -3
    torch.cuda.synchronize()
    for name, (a, g) in o.host().items():                                        # nothing was queued
        pattern = NAN_BITS if name in Outputs.F64 else INT_GUARD
        assert np.all(a == pattern) and np.all(g == pattern), name
