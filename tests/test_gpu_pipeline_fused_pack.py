"""
GPU tests of the pipelines' `fused_pack` (spinrelax_amd/pipeline.py, _PlaneRing.pack_in_ct): the C(t) launch of batch k carries the
pack of batch k + 1.  A FEED hands out a different shard for every batch -- with one repeated shard a pack that lands in the wrong
plane buffer, or before the buffer's readers are done, would not show -- and every batch's C(t), dC(t), histogram and result
arrays must be the bits the stand-alone pack on the auxiliary stream gives.  V = 32, R = 2, F = 4096: the cfg3 / cfg4 kernel.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V, R, F, NB_BATCHES = 32, 2, 4096, 7
FRAMES = R * F + 8          # Npad = 8256: the planes have a padded tail


class Feed:
    """a different device array per batch; records what the pipeline asks of it"""

    def __init__(self, shards):
        self.shards = shards
        self.V = shards[0].shape[1]
        self.log = []

    def acquire(self, k, stream):
        self.log.append(('acquire', k))
        return self.shards[k]

    def release(self, k, stream):
        self.log.append(('release', k))


@pytest.fixture(scope='module')
def st():
    import torch
    from spinrelax_amd import synth
    from spinrelax_amd.hip import Context
    ctx = Context(0)
    dev = torch.device('cuda', 0)
    # seven shards of one synthetic trajectory family (ordered vectors: the fits converge quickly), each its own seed
    shards = [torch.from_numpy(synth.synth_vectors(FRAMES, V, seed=100 + k)).to(dev) for k in range(NB_BATCHES)]
    kw = dict(q_rot=synth.Q_EXT, Diso=synth.DISO, aniso=synth.DANI, field_MHz=(synth.FIELD_MHZ,), zeta=synth.ZETA)
    cache = {}
    yield dict(torch=torch, ctx=ctx, dev=dev, shards=shards, kw=kw, dt=synth.config_shapes(3)['dt'], cache=cache)
    ctx.close()


def run(st, kind, fused, plane_buffers):
    """every batch's outputs and the feed's log; the stand-alone runs are shared between the tests"""
    key = (kind, fused, plane_buffers)
    if key in st['cache']:
        return st['cache'][key]
    from spinrelax_amd.pipeline import DevicePipeline, GroupedPipeline
    torch = st['torch']
    feed = Feed(st['shards'])
    common = dict(stream=torch.cuda.Stream(device=st['dev']), plane_buffers=plane_buffers, fused_pack=fused, **st['kw'])
    if kind == 'grouped':
        pipe = GroupedPipeline(st['ctx'], st['dev'], FRAMES, V, R, F, st['dt'], group=3, **common)
    else:
        pipe = DevicePipeline(st['ctx'], st['dev'], FRAMES, V, R, F, st['dt'], depth=3, **common)
    assert pipe.fused_pack is fused
    out, snaps = [], []
    side = torch.cuda.Stream(device=st['dev'])

    def on_finished(b):
        d = {k: np.array(v, copy=True) for k, v in b.result.items()}
        if kind == 'grouped':                   # a group's device arrays stay until its buffer is taken again, two groups later
            d.update(Ct=b.Ct.cpu().numpy(), dCt=b.dCt.cpu().numpy(), hist=b.hist.cpu().numpy())
        out.append(d)

    def on_enqueued(slot):
        """per-batch schedule: the next tenant of the slot may overwrite its histogram before on_finished runs -- a device-side
        reader queued behind the batch takes the arrays, and the pipeline waits for the event returned"""
        with torch.cuda.stream(side):
            side.wait_event(slot.done)
            snaps.append((slot.Ct.clone(), slot.dCt.clone(), slot.hist.clone()))
            ev = torch.cuda.Event()
            ev.record(side)
        return ev
    pipe.run(feed, NB_BATCHES, None, on_finished, on_enqueued if kind == 'device' else None)
    torch.cuda.synchronize()
    for d, snap in zip(out, snaps):
        d.update(Ct=snap[0].cpu().numpy(), dCt=snap[1].cpu().numpy(), hist=snap[2].cpu().numpy())
    pipe.close()
    assert len(out) == NB_BATCHES
    st['cache'][key] = (out, feed.log)
    return out, feed.log


def check_feed_log(log):
    for k in range(NB_BATCHES):
        assert log.count(('acquire', k)) == 1 and log.count(('release', k)) == 1, (k, log)
        assert log.index(('acquire', k)) < log.index(('release', k)), (k, log)


@pytest.mark.parametrize('kind,plane_buffers', [('grouped', 3), ('device', 3), ('grouped', 2), ('device', 2)])
def test_every_batch_is_the_same_with_the_pack_carried(st, kind, plane_buffers):
    off, log_off = run(st, kind, False, plane_buffers)
    on, log_on = run(st, kind, True, plane_buffers)
    check_feed_log(log_off)
    check_feed_log(log_on)
    for k, (a, b) in enumerate(zip(off, on)):
        assert set(a) == set(b)
        for name in a:
            assert np.array_equal(a[name], b[name], equal_nan=True), (k, name)
    # the shards differ, and so do their results: a pack in the wrong buffer could not hide
    assert not np.array_equal(off[0]['Ct'], off[1]['Ct'])
    assert not np.array_equal(off[NB_BATCHES - 1]['hist'], off[NB_BATCHES - 2]['hist'])


@pytest.mark.parametrize('plane_buffers,alone', [(3, 2), (2, 1)])
def test_the_launches_carry_the_pack(st, plane_buffers, alone):
    """with fused_pack the pipeline asks the library, and the library says yes for this shape.  The ring holds one buffer more than
    asked for; with four, a C(t) launch packs the batch after the next (the next launch of its own stream) and a run's first two
    batches are packed alone, with three it packs the next batch and only the first is packed alone"""
    from spinrelax_amd.pipeline import GroupedPipeline
    torch, ctx = st['torch'], st['ctx']
    pipe = GroupedPipeline(ctx, st['dev'], FRAMES, V, R, F, st['dt'], group=3, fused_pack=True, plane_buffers=plane_buffers,
                           stream=torch.cuda.Stream(device=st['dev']), **st['kw'])
    assert pipe.ring.NB == plane_buffers + 1 and pipe.ring.reach == (2 if plane_buffers == 3 else 1)
    calls = {'pack': 0, 'carried': 0}
    pack, carry = ctx.pack_soa_dev, ctx.ct_sums_pack_dev

    def count_pack(*a):
        calls['pack'] += 1
        return pack(*a)

    def count_carry(*a):
        calls['carried'] += 1
        return carry(*a)
    ctx.pack_soa_dev, ctx.ct_sums_pack_dev = count_pack, count_carry
    feed = Feed(st['shards'])
    try:
        pipe.run(feed, NB_BATCHES)
        torch.cuda.synchronize()
    finally:
        del ctx.pack_soa_dev, ctx.ct_sums_pack_dev
        pipe.close()
    assert calls == {'pack': alone, 'carried': NB_BATCHES - alone}
    assert [k for what, k in feed.log if what == 'acquire'] == list(range(NB_BATCHES))       # a feed is asked for its batches in order
