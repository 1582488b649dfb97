#!/usr/bin/env python3
"""Developer timing of k_ct_dipolar_cross against k_ct_cross on the same pairs in the same run -- NPAIR pairs (default 512) x the chunks
of cfg3 (24 x 4096 frames; CFG=2: cfg2's) --, in one process on one device; docs/EXPERIMENTS.md section 24.  The vectors are cfg3's unit
vectors, for the dipolar call times a distance 0.3 exp(0.1 g), g standard normal.  Per figure: device events around CALLS (default 20)
back-to-back calls after a warm-up call, the best of ROUNDS (default 3) rounds, per call; the two kernels alternate round by round.
Both calls upload their small tables and run k_ct_cross_p0 and k_ct_finalize, the dipolar one also its normalisation kernel: kernel
times alone come from running this script under `rocprofv3 --kernel-trace --stats`.  Per (t, lag) and direction the dipolar kernel issues
5 FMAs against 4: the counts give a ratio of 1.25; the gate is 1.5 on the symmetric form (exit status 1 above it)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from spinrelax_amd import synth                      # noqa: E402
from spinrelax_amd.hip import Context                # noqa: E402

PEAK_FP32 = 157.3e12                                 # MI355X vector FP32, FLOP/s (an FMA counts two)
GATE = 1.5

s = synth.config_shapes(int(os.environ.get('CFG', '3')))
V = int(os.environ.get('NPAIR', '512'))
CALLS, ROUNDS = int(os.environ.get('CALLS', '20')), int(os.environ.get('ROUNDS', '3'))
R, F, L = s['R'], s['F'], s['F'] // 2
pre = synth.synth_vectors_parallel(s['frames'], V, s['seed'])
ctx = Context(0)
vecs = torch.from_numpy(pre).cuda()
Npad = (s['frames'] + 63) // 64 * 64
soa = torch.empty((V, 3, Npad), device='cuda', dtype=torch.float32)
ctx.pack_soa_dev(vecs.data_ptr(), s['frames'], V, 0, V, soa.data_ptr(), Npad)
gen = torch.Generator(device='cuda').manual_seed(s['seed'])
dist = (0.3 * torch.exp(0.1 * torch.randn((s['frames'], V), device='cuda', generator=gen))).to(torch.float32)
soa4 = torch.empty((V, 4, Npad), device='cuda', dtype=torch.float32)
rref = torch.empty((V,), device='cuda', dtype=torch.float64)
ctx.pack_dipolar_dev(vecs.data_ptr(), dist.data_ptr(), s['frames'], V, 0, V, soa4.data_ptr(), Npad, rref.data_ptr())
psum = torch.empty((V * R * ctx.psum_stride(F),), device='cuda', dtype=torch.float64)
P0 = torch.empty((2, V), device='cuda', dtype=torch.float64)
Ct = torch.empty((L, V), device='cuda', dtype=torch.float64)
dCt = torch.empty((L, V), device='cuda', dtype=torch.float64)
ws = torch.empty((V, R, 2), device='cuda', dtype=torch.float64)
pairs = np.stack((np.arange(V), (np.arange(V) + 1) % V), axis=1)


def cross(sym):
    ctx.ct_cross_dev(soa.data_ptr(), Npad, V, R, F, pairs, P0[0].data_ptr(), Ct.data_ptr(), dCt.data_ptr(), sym=sym, psum_ptr=psum.data_ptr(),
                     dP0_ptr=P0[1].data_ptr())


def dipolar(sym):
    ctx.ct_dipolar_cross_dev(soa4.data_ptr(), Npad, V, R, F, pairs, P0[0].data_ptr(), Ct.data_ptr(), dCt.data_ptr(), ws.data_ptr(), sym=sym,
                             psum_ptr=psum.data_ptr(), dP0_ptr=P0[1].data_ptr())


cases = [(cross, 1), (dipolar, 1), (cross, 0), (dipolar, 0)]
best = {c: np.inf for c in cases}
for _ in range(ROUNDS):
    for fn, sym in cases:
        fn(sym)                                      # warm-up
        ctx.sync()
        ctx.timer_start()
        for _ in range(CALLS):
            fn(sym)
        best[(fn, sym)] = min(best[(fn, sym)], ctx.timer_stop_ms() / CALLS)
dipolar(1)
ctx.sync()
checksum = float(Ct.sum().item())
trip = synth.exact_triples(R, F, V)                  # (t, lag) products of one direction, lags 1 .. L
print('R=%d F=%d pairs=%d  best of %d x %d calls, ms per call' % (R, F, V, ROUNDS, CALLS))
for sym in (1, 0):
    tc, td = best[(cross, sym)], best[(dipolar, sym)]
    fd = 10.0 * trip * (1 + sym)                     # 5 FMAs per product and direction
    print('sym=%d  k_ct_cross %.3f ms   k_ct_dipolar_cross %.3f ms  %.1f TFLOP/s = %.1f %% of the FP32 vector peak   ratio %.3f' %
          (sym, tc, td, fd / td * 1e-9, 100.0 * fd / (td * 1e-3) / PEAK_FP32, td / tc))
ratio = best[(dipolar, 1)] / best[(cross, 1)]
print('ratio sym=1 %.3f (gate %.2f)   checksum %.12g' % (ratio, GATE, checksum))
ctx.close()
sys.exit(0 if ratio <= GATE else 1)
