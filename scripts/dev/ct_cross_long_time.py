#!/usr/bin/env python3
"""Developer timing of the pair cross-correlation call at chunk lengths around and beyond what k_ct_cross can stage: the blocked form
(sr_ct_cross_long.hip) against the staged kernel where both run (F = 6000), and against its compulsory HBM traffic where only the
blocked form does (F = 25 000, 100 000); docs/EXPERIMENTS.md section 21.

    python scripts/dev/ct_cross_long_time.py [--npair 512] [--reps 7] [--json FILE]

512 pairs (v, v + 1) of 512 vectors, sym = 1, one chunk per vector (R = 1).  One child process per chunk length, each under its own
time limit; the run stops at the first child that fails.  Inside a child: planes packed once, one warm-up call, then the median of
--reps calls timed with HIP events on the context's stream.  A call is the whole entry point (sr_ct_cross_f32_dev /
sr_ct_cross_long_f32_dev): the upload of the pair table, the kernels, k_ct_cross_p0 and k_ct_finalize.  The two entry points are
called directly; spinrelax_amd/ct.py chooses between them by "ct_cross_long_min_frames", which this table is there to inform.
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

BOTH = (6000,)                           # the staged kernel runs too
LONG = (25000, 100000)                   # blocked only
B = 4096


def one(F, V, reps, with_direct):
    import numpy as np
    import torch
    from spinrelax_amd import synth
    from spinrelax_amd.hip import Context
    pre = synth.synth_vectors(F, V, seed=900 + F % 97)          # in this process, before the GPU is initialised: no forked workers
    ctx = Context(0)
    Npad = (F + 63) // 64 * 64
    L = F // 2
    vecs = torch.from_numpy(pre).cuda()
    soa = torch.empty((V, 3, Npad), device='cuda', dtype=torch.float32)
    psum = torch.empty((V * ctx.psum_stride(F),), device='cuda', dtype=torch.float64)
    P0 = torch.empty((V,), device='cuda', dtype=torch.float64)
    Ct = torch.empty((L, V), device='cuda', dtype=torch.float64)
    dCt = torch.empty((L, V), device='cuda', dtype=torch.float64)
    ctx.pack_soa_dev(vecs.data_ptr(), F, V, 0, V, soa.data_ptr(), Npad)
    pairs = np.stack((np.arange(V), (np.arange(V) + 1) % V), axis=1)
    res = {'F': F, 'pairs': V}
    for tag, fn in (('blocked', ctx.ct_cross_long_dev),) + ((('direct', ctx.ct_cross_dev),) if with_direct else ()):
        def call():
            fn(soa.data_ptr(), Npad, V, 1, F, pairs, P0.data_ptr(), Ct.data_ptr(), dCt.data_ptr(), sym=1, psum_ptr=psum.data_ptr())
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
    # compulsory HBM traffic of the blocked form: the planes once, the block spectra (five signals) written once and read once
    nb = -(-F // B)
    res['hbm_bytes'] = V * (12 * F + 2 * 5 * nb * 4097 * 8)
    res['hbm_GBps'] = res['hbm_bytes'] / res['blocked_ms'] / 1e6
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--npair', type=int, default=512)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--json', default=None)
    ap.add_argument('--one', type=int, default=None, help='(child) time this chunk length and print one JSON line')
    ap.add_argument('--direct', type=int, default=0)
    a = ap.parse_args()
    if a.one is not None:
        print('RESULT ' + json.dumps(one(a.one, a.npair, a.reps, bool(a.direct))), flush=True)
        return 0
    rows = []
    for F in BOTH + LONG:
        cmd = [sys.executable, os.path.abspath(__file__), '--one', str(F), '--npair', str(a.npair), '--reps', str(a.reps),
               '--direct', '1' if F in BOTH else '0']
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
        except subprocess.TimeoutExpired:
            print('F=%d: time limit; stopping' % F)
            return 1
        txt = p.stdout.decode()
        if p.returncode != 0:
            print('F=%d: exit status %d; stopping\n%s' % (F, p.returncode, txt))
            return 1
        r = json.loads([ln for ln in txt.splitlines() if ln.startswith('RESULT ')][-1][7:])
        rows.append(r)
        if 'direct_ms' in r:
            print('F=%6d  blocked %8.3f ms (min %.3f)  direct %8.3f ms (min %.3f)  direct/blocked %5.2f' % (
                F, r['blocked_ms'], r['blocked_min_ms'], r['direct_ms'], r['direct_min_ms'], r['direct_ms'] / r['blocked_ms']), flush=True)
        else:
            print('F=%6d  blocked %8.3f ms (min %.3f)  compulsory HBM traffic %.2f GB -> %.0f GB/s' % (
                F, r['blocked_ms'], r['blocked_min_ms'], r['hbm_bytes'] / 1e9, r['hbm_GBps']), flush=True)
    if a.json:
        with open(a.json, 'w') as fp:
            json.dump(rows, fp, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
