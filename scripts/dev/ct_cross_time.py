#!/usr/bin/env python3
"""Developer timing of k_ct_cross (NPAIR pairs, SYM = 1 | 0) against k_ct_palmer (NPAIR vectors, ct_fft = 0) on the cfg3 planes
(CFG=2: cfg2's), the same R and F, alternating, device events around each call; docs/EXPERIMENTS.md section 20.  The cross call
also uploads its pair table and runs k_ct_cross_p0 and k_ct_finalize: kernel times alone come from running this script under
`rocprofv3 --kernel-trace --stats`."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from spinrelax_amd import synth                      # noqa: E402
from spinrelax_amd.hip import Context                # noqa: E402

s = synth.config_shapes(int(os.environ.get('CFG', '3')))
V = int(os.environ.get('NPAIR', '512'))
sym = int(os.environ.get('SYM', '1'))
R, F, L = s['R'], s['F'], s['F'] // 2
pre = synth.synth_vectors_parallel(s['frames'], V, s['seed'])
ctx = Context(0)
ctx.set_option('ct_fft', 0)                          # kernel 1 in its direct form: k_ct_palmer
vecs = torch.from_numpy(pre).cuda()
Npad = (s['frames'] + 63) // 64 * 64
soa = torch.empty((V, 3, Npad), device='cuda', dtype=torch.float32)
psum = torch.empty((V * R * ctx.psum_stride(F),), device='cuda', dtype=torch.float64)
P0 = torch.empty((V,), device='cuda', dtype=torch.float64)
Ct = torch.empty((L, V), device='cuda', dtype=torch.float64)
dCt = torch.empty((L, V), device='cuda', dtype=torch.float64)
ctx.pack_soa_dev(vecs.data_ptr(), s['frames'], V, 0, V, soa.data_ptr(), Npad)
pairs = np.stack((np.arange(V), (np.arange(V) + 1) % V), axis=1)


def auto():
    ctx.ct_sums_dev(soa.data_ptr(), Npad, R, F, V, psum.data_ptr())


def cross():
    ctx.ct_cross_dev(soa.data_ptr(), Npad, V, R, F, pairs, P0.data_ptr(), Ct.data_ptr(), dCt.data_ptr(), sym=sym, psum_ptr=psum.data_ptr())


for fn in (auto, cross):
    fn()
ctx.sync()
ts = {auto: [], cross: []}
for _ in range(int(os.environ.get('REPS', '9'))):
    for fn in (auto, cross):
        ctx.timer_start()
        fn()
        ts[fn].append(ctx.timer_stop_ms())
ta, tc = float(np.median(ts[auto])), float(np.median(ts[cross]))
flop = 8.0 * synth.exact_triples(R, F, V)            # 3 FMA for the dot product, 1 for the square-accumulate, lags 1 .. L
print('R=%d F=%d N=%d  k_ct_palmer median %.3f ms (min %.3f) %.1f TFLOP/s   ct_cross sym=%d median %.3f ms (min %.3f) %.1f TFLOP/s   ratio %.2f   '
      'checksum %.12g' % (R, F, V, ta, min(ts[auto]), flop / ta * 1e-9, sym, tc, min(ts[cross]), (1 + sym) * flop / tc * 1e-9, tc / ta,
                          float(Ct.sum().item())))
ctx.close()
