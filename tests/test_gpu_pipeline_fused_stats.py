"""
GPU tests of GroupedPipeline's `fused_stats` (spinrelax_amd/pipeline.py): the merged search launch computes the chunk statistics of
its residues from the raw sums, and no k_ct_finalize launch runs per batch.  V = 8, R = 3, F = 512, groups of 2, five batches (groups
2, 2, 1): once fed with a different shard per batch, once with one device tensor.  Every batch's C(t), dC(t) in both orientations,
histogram, selected models and table must be the bits the per-batch launches give; on_part('ct') fires once per batch, in batch order,
with an event that covers the data; with `dev_skip_fits` the per-batch path runs and the pipeline says so.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V, R, F, GROUP, NB_BATCHES = 8, 3, 512, 2, 5
FRAMES = R * F


class Feed:
    def __init__(self, shards):
        self.shards = shards
        self.V = shards[0].shape[1]

    def acquire(self, k, stream):
        return self.shards[k]

    def release(self, k, stream):
        pass


@pytest.fixture(scope='module')
def st():
    import torch
    from spinrelax_amd import synth
    from spinrelax_amd.hip import Context
    ctx = Context(0)
    dev = torch.device('cuda', 0)
    shards = [torch.from_numpy(synth.synth_vectors(FRAMES, V, seed=300 + k)).to(dev) for k in range(NB_BATCHES)]
    kw = dict(q_rot=synth.Q_EXT, Diso=synth.DISO, aniso=synth.DANI, field_MHz=(synth.FIELD_MHZ,), zeta=synth.ZETA)
    yield dict(torch=torch, ctx=ctx, dev=dev, shards=shards, kw=kw, dt=synth.config_shapes(3)['dt'], cache={})
    ctx.close()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def make(st, fused):
    from spinrelax_amd.pipeline import GroupedPipeline
    return GroupedPipeline(st['ctx'], st['dev'], FRAMES, V, R, F, st['dt'], group=GROUP, fused_stats=fused,
                           stream=st['torch'].cuda.Stream(device=st['dev']), **st['kw'])


def run(st, source, fused):
    """every batch's outputs, what on_part saw, and the library calls the run made; shared between the tests"""
    key = (source, fused)
    if key in st['cache']:
        return st['cache'][key]
    torch, ctx = st['torch'], st['ctx']
    pipe = make(st, fused)
    assert pipe.fused_stats is fused and (pipe.fused_stats_note is None) == fused
    assert pipe.group_sizes(NB_BATCHES) == [2, 2, 1]
    vecs = Feed(st['shards']) if source == 'feed' else st['shards'][0]
    out, parts = [], []
    side = torch.cuda.Stream(device=st['dev'])
    calls = {'finalize': 0, 'sums': 0, 'batched': 0, 'transpose': 0}
    names = {'finalize': 'ct_finalize_dev', 'sums': 'order_search_sums_dev', 'batched': 'order_search_batched_dev',
             'transpose': 'transpose_batched_dev'}

    def counted(what, fn):
        def f(*a, **k):
            calls[what] += 1
            return fn(*a, **k)
        return f
    for what, name in names.items():
        setattr(ctx, name, counted(what, getattr(ctx, name)))

    def on_part(kind, bv, ev):
        if kind != 'ct':
            return
        # the event covers the data: a stream that waited for it reads C(t), dC(t) of the batch
        with torch.cuda.stream(side):
            side.wait_event(ev)
            parts.append((bv.index, bv.Ct.clone(), bv.dCt.clone()))

    def on_finished(b):
        d = {k: np.array(v, copy=True) for k, v in b.result.items()}
        d.update(Ct=b.Ct.cpu().numpy(), dCt=b.dCt.cpu().numpy(), CtT=b.CtT.cpu().numpy(), dCtT=b.dCtT.cpu().numpy(),
                 hist=b.hist.cpu().numpy())
        out.append(d)

    def on_enqueued(grp):
        """the side stream's reads of the group are ordered before the pipeline overwrites its buffers"""
        ev = torch.cuda.Event()
        ev.record(side)
        return ev
    try:
        pipe.run(vecs, NB_BATCHES, None, on_finished, on_enqueued, on_part)
        torch.cuda.synchronize()
    finally:
        for name in names.values():
            delattr(ctx, name)
    still = pipe.fused_stats
    pipe.close()
    parts = [(j, a.cpu().numpy(), b.cpu().numpy()) for j, a, b in parts]
    st['cache'][key] = (out, parts, calls, still)
    return st['cache'][key]


@pytest.mark.parametrize('source', ['feed', 'tensor'])
def test_every_batch_is_the_same_with_the_statistics_fused(st, source):
    off, parts_off, calls_off, _ = run(st, source, False)
    on, parts_on, calls_on, still = run(st, source, True)
    assert still                                         # the library took the call: no fallback on the way
    assert len(off) == len(on) == NB_BATCHES
    for k, (a, b) in enumerate(zip(off, on)):
        assert set(a) == set(b) and {'Ct', 'dCt', 'CtT', 'dCtT', 'hist', 'relax', 'best', 'S2', 'C', 'tau', 'K', 'chi'} <= set(a)
        for name in a:
            assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, (k, name)
            assert np.array_equal(bits(a[name]), bits(b[name])), (k, name)
        assert np.array_equal(a['CtT'], a['Ct'].T) and np.array_equal(b['dCtT'], b['dCt'].T)
        assert np.all(np.isfinite(b['Ct'])) and np.all(b['dCt'] > 0)
    # one merged launch and one pair of transpositions per group, no per-batch launch -- and the other way round
    assert calls_on == {'finalize': 0, 'sums': 3, 'batched': 0, 'transpose': 6}
    assert calls_off == {'finalize': NB_BATCHES, 'sums': 0, 'batched': 3, 'transpose': 0}
    if source == 'feed':       # the shards differ, and so do their results: a batch in the wrong row of the group could not hide
        assert not np.array_equal(on[0]['Ct'], on[1]['Ct']) and not np.array_equal(on[3]['Ct'], on[4]['Ct'])


@pytest.mark.parametrize('source', ['feed', 'tensor'])
@pytest.mark.parametrize('fused', [True, False])
def test_on_part_ct_fires_once_per_batch_in_order_and_its_event_covers_the_data(st, source, fused):
    out, parts, _, _ = run(st, source, fused)
    assert [j for j, _, _ in parts] == [0, 1, 0, 1, 0]           # index inside the group: groups 2, 2, 1, batch order
    for d, (_, Ct, dCt) in zip(out, parts):
        assert np.array_equal(bits(Ct), bits(d['Ct'])) and np.array_equal(bits(dCt), bits(d['dCt']))


def test_dev_skip_fits_takes_the_per_batch_launches_and_says_so(st):
    torch, ctx = st['torch'], st['ctx']
    want, _, _, _ = run(st, 'tensor', False)
    pipe = make(st, True)
    assert pipe.fused_stats is True and pipe.fused_stats_note is None
    pipe.dev_skip_fits = True
    assert pipe.fused_stats is False and 'dev_skip_fits' in pipe.fused_stats_note
    calls = {'finalize': 0, 'sums': 0}
    fin, sums = ctx.ct_finalize_dev, ctx.order_search_sums_dev

    def count_fin(*a, **k):
        calls['finalize'] += 1
        return fin(*a, **k)

    def count_sums(*a, **k):
        calls['sums'] += 1
        return sums(*a, **k)
    ctx.ct_finalize_dev, ctx.order_search_sums_dev = count_fin, count_sums
    got = []
    try:
        pipe.run(st['shards'][0], 3, None, lambda b: got.append((b.Ct.cpu().numpy(), b.dCt.cpu().numpy())))
        torch.cuda.synchronize()
    finally:
        del ctx.ct_finalize_dev, ctx.order_search_sums_dev
        pipe.close()
    assert calls == {'finalize': 3, 'sums': 0} and len(got) == 3
    for Ct, dCt in got:
        assert np.array_equal(Ct, want[0]['Ct']) and np.array_equal(dCt, want[0]['dCt'])
