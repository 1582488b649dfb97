#!/usr/bin/env python3
"""Developer timing of the blocked forms of the two distance-weighted correlation functions (sr_ct_dipolar_long.hip);
docs/EXPERIMENTS.md section 28.

    python scripts/dev/ct_dipolar_long_time.py [--nvec 512] [--chunks 5] [--reps 5] [--json FILE]

Four measurements, one child process each, each under its own time limit; the run stops at the first child that fails:
  auto 20000   --nvec vectors x --chunks chunks of 20 000 frames: the blocked C_dd(t) beside the blocked C(t) of kernel 1 on unit vectors
               of the same shape (both transform five signals per series: a ratio well above 1 would need explaining)
  pair 20000   --nvec pairs (v, v + 1) on the same shape, sym = 1: the blocked pair form beside the blocked --crossCt on unit vectors
  auto 10016   the longest chunk k_ct_dipolar stages: blocked against direct
  pair 4896    the longest chunk k_ct_dipolar_cross stages: blocked against direct
Inside a child: planes packed once, one warm-up call, then the median of --reps calls timed with HIP events on the context's stream.  A
call is the whole _dev entry point.  The entry points are called directly; spinrelax_amd/ct.py chooses between them by
"ct_dipolar_long_min_frames" / "ct_dipolar_cross_long_min_frames", which the last two rows are there to inform.
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

CASES = (('auto', 20000), ('pair', 20000), ('auto', 10016), ('pair', 4896))


def one(kind, F, V, R, reps):
    import numpy as np
    import torch
    from spinrelax_amd import synth
    from spinrelax_amd.hip import Context
    N = R * F
    unit = synth.synth_vectors(N, V, seed=900 + F % 97)         # in this process, before the GPU is initialised: no forked workers
    rng = np.random.default_rng(F)
    dist = (0.3 * np.exp(0.1 * rng.standard_normal((N, V)))).astype(np.float32)
    ctx = Context(0)
    Npad = (N + 63) // 64 * 64
    L = F // 2
    vecs = torch.from_numpy(unit).cuda()
    dd = torch.from_numpy(dist).cuda()
    soa = torch.empty((V, 3, Npad), device='cuda', dtype=torch.float32)
    soa4 = torch.empty((V, 4, Npad), device='cuda', dtype=torch.float32)
    rref = torch.empty((V,), device='cuda', dtype=torch.float64)
    psum = torch.empty((V * R * ctx.psum_stride(F),), device='cuda', dtype=torch.float64)
    P0 = torch.empty((2, V), device='cuda', dtype=torch.float64)
    Ct = torch.empty((L, V), device='cuda', dtype=torch.float64)
    dCt = torch.empty((L, V), device='cuda', dtype=torch.float64)
    wm = torch.empty((V, R, 2), device='cuda', dtype=torch.float64)
    ctx.pack_soa_dev(vecs.data_ptr(), N, V, 0, V, soa.data_ptr(), Npad)
    ctx.pack_dipolar_dev(vecs.data_ptr(), dd.data_ptr(), N, V, 0, V, soa4.data_ptr(), Npad, rref.data_ptr())
    ctx.sync()
    del vecs, dd
    pairs = np.stack((np.arange(V), (np.arange(V) + 1) % V), axis=1)
    pp, cc, dc, ww, ps = P0[0].data_ptr(), Ct.data_ptr(), dCt.data_ptr(), wm.data_ptr(), psum.data_ptr()
    if kind == 'auto':
        calls = [('dipolar_blocked', lambda: ctx.ct_dipolar_long_dev(soa4.data_ptr(), Npad, V, R, F, cc, dc, ww, psum_ptr=ps))]
        if F > ctx.ct_dipolar_max_frames():
            calls.append(('unit_blocked', lambda: ctx.ct_palmer_dev(soa.data_ptr(), Npad, R, F, V, cc, dc, psum_ptr=ps)))
        else:
            calls.append(('dipolar_direct', lambda: ctx.ct_dipolar_dev(soa4.data_ptr(), Npad, V, R, F, cc, dc, ww, psum_ptr=ps)))
    else:
        calls = [('dipolar_blocked', lambda: ctx.ct_dipolar_cross_long_dev(soa4.data_ptr(), Npad, V, R, F, pairs, pp, cc, dc, ww, sym=1, psum_ptr=ps))]
        if F > ctx.ct_dipolar_cross_max_frames():
            calls.append(('unit_blocked', lambda: ctx.ct_cross_long_dev(soa.data_ptr(), Npad, V, R, F, pairs, pp, cc, dc, sym=1, psum_ptr=ps)))
        else:
            calls.append(('dipolar_direct', lambda: ctx.ct_dipolar_cross_dev(soa4.data_ptr(), Npad, V, R, F, pairs, pp, cc, dc, ww, sym=1, psum_ptr=ps)))
    res = {'kind': kind, 'F': F, 'rows': V, 'chunks': R}
    for tag, call in calls:
        call()
        ctx.sync()
        ts = []
        for _ in range(reps):
            ctx.timer_start()
            call()
            ts.append(ctx.timer_stop_ms())
        res[tag + '_ms'] = float(np.median(ts))
        res[tag + '_min_ms'] = float(min(ts))
        res[tag + '_checksum'] = float(Ct.sum().item())
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nvec', type=int, default=512)
    ap.add_argument('--chunks', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--one', default=None, help='(child) kind:F -- time this case and print one JSON line')
    a = ap.parse_args()
    if a.one is not None:
        kind, F = a.one.split(':')
        print('RESULT ' + json.dumps(one(kind, int(F), a.nvec, a.chunks, a.reps)), flush=True)
        return 0
    rows = []
    for kind, F in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), '--one', '%s:%d' % (kind, F), '--nvec', str(a.nvec), '--chunks', str(a.chunks),
               '--reps', str(a.reps)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        except subprocess.TimeoutExpired:
            print('%s F=%d: time limit; stopping' % (kind, F))
            return 1
        txt = p.stdout.decode()
        if p.returncode != 0:
            print('%s F=%d: exit status %d; stopping\n%s' % (kind, F, p.returncode, txt))
            return 1
        r = json.loads([ln for ln in txt.splitlines() if ln.startswith('RESULT ')][-1][7:])
        rows.append(r)
        other = 'unit_blocked' if 'unit_blocked_ms' in r else 'dipolar_direct'
        print('%s F=%6d  dipolar blocked %9.3f ms (min %.3f)  %s %9.3f ms (min %.3f)  dipolar blocked / %s %5.2f' % (
            kind, F, r['dipolar_blocked_ms'], r['dipolar_blocked_min_ms'], other.replace('_', ' '), r[other + '_ms'], r[other + '_min_ms'],
            other.replace('_', ' '), r['dipolar_blocked_ms'] / r[other + '_ms']), flush=True)
    if a.json:
        with open(a.json, 'w') as fp:
            json.dump(rows, fp, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
