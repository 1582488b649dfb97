#!/usr/bin/env python3
"""Developer timing of the C(t) raw-sums call alone at chunk lengths beyond one in-LDS transform: the blocked kernels of the
default dispatch (sr_ct_long.hip) against the direct kernel (ct_fft = 0) where both run, and against the compulsory HBM
traffic where only the blocked form does.

    python scripts/dev/ct_long_timing.py [--nvec 512] [--reps 7] [--json FILE]

One child process per chunk length, each under its own time limit; the run stops at the first child that fails.  Inside a
child: one chunk per vector (R = 1), planes packed once, one warm-up call, then the median of --reps calls timed with HIP
events on the context's stream (the blocked form is forced below the direct kernel's limit with "ct_long_min_frames" = 5462).
Switch point of the dispatch: the blocked form takes a length when it is the faster one; set SR_CT_LONG_MIN_FRAMES from this table.
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

BOTH = (5462, 8192, 10000, 13000)        # the direct kernel runs too
LONG = (25000, 40000)                    # blocked only
B = 4096


def one(F, V, reps, with_direct):
    import numpy as np
    import torch
    from spinrelax_amd import synth
    from spinrelax_amd.hip import Context
    pre = synth.synth_vectors(F, V, seed=900 + F % 97)          # in this process, before the GPU is initialised: no forked workers
    ctx = Context(0)
    Npad = (F + 63) // 64 * 64
    vecs = torch.from_numpy(pre).cuda()
    soa = torch.empty((V, 3, Npad), device='cuda', dtype=torch.float32)
    psum = torch.empty((V * ctx.psum_stride(F),), device='cuda', dtype=torch.float64)
    ctx.pack_soa_dev(vecs.data_ptr(), F, V, 0, V, soa.data_ptr(), Npad)
    res = {'F': F, 'V': V}
    for tag, opt in (('blocked', {'ct_fft': 3, 'ct_long_min_frames': 5462}),) + ((('direct', {'ct_fft': 0}),) if with_direct else ()):
        for k, v in opt.items():
            ctx.set_option(k, v)
        ctx.ct_sums_dev(soa.data_ptr(), Npad, 1, F, V, psum.data_ptr())
        ctx.sync()
        ts = []
        for _ in range(reps):
            ctx.timer_start()
            ctx.ct_sums_dev(soa.data_ptr(), Npad, 1, F, V, psum.data_ptr())
            ts.append(ctx.timer_stop_ms())
        res[tag + '_ms'] = float(np.median(ts))
        res[tag + '_min_ms'] = float(min(ts))
    # compulsory HBM traffic of the blocked form: the planes read three times (constants, scan, spectra: 2 to 3 planes per
    # signal come from the caches), the block spectra written and read once, the cross-spectra written and read once
    nb, nd = -(-F // B), F // 2 // B + 1
    res['hbm_bytes'] = V * (3 * 12 * F + 2 * 5 * nb * 4097 * 8 + 2 * nd * 4097 * 16)
    res['hbm_GBps'] = res['hbm_bytes'] / res['blocked_ms'] / 1e6
    # float32 transform work: 5 nb real-input transforms of 8192 points, 2.5 M log2 M flops each
    res['fft_flops'] = V * 5 * nb * 2.5 * 8192 * 13
    res['fft_TFLOPs'] = res['fft_flops'] / res['blocked_ms'] / 1e9
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nvec', type=int, default=512)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--json', default=None)
    ap.add_argument('--one', type=int, default=None, help='(child) time this chunk length and print one JSON line')
    ap.add_argument('--direct', type=int, default=0)
    a = ap.parse_args()
    if a.one is not None:
        print('RESULT ' + json.dumps(one(a.one, a.nvec, a.reps, bool(a.direct))), flush=True)
        return 0
    rows = []
    for F in BOTH + LONG:
        cmd = [sys.executable, os.path.abspath(__file__), '--one', str(F), '--nvec', str(a.nvec), '--reps', str(a.reps),
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
            print('F=%6d  blocked %8.3f ms  direct %8.3f ms  direct/blocked %5.2f' % (F, r['blocked_ms'], r['direct_ms'],
                                                                                       r['direct_ms'] / r['blocked_ms']), flush=True)
        else:
            print('F=%6d  blocked %8.3f ms  compulsory HBM traffic %.2f GB -> %.0f GB/s, float32 transforms %.1f TFLOP/s' % (
                F, r['blocked_ms'], r['hbm_bytes'] / 1e9, r['hbm_GBps'], r['fft_TFLOPs']), flush=True)
    if a.json:
        with open(a.json, 'w') as fp:
            json.dump(rows, fp, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
