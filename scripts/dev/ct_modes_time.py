#!/usr/bin/env python3
"""Developer timing of k_ct_modes against k_ct_palmer (direct form, ct_fft = 0) and k_ct_dipolar on the same shape -- NVEC vectors
(default 512) x the chunks of cfg3 (24 x 4096 frames; CFG=2: cfg2's) --, alternating in one process on one device, device events around
each call; docs/EXPERIMENTS.md section 37.  The vectors are cfg3's unit vectors (the dipolar call: times a distance 0.3 exp(0.1 g), g
standard normal), the frame a generic quaternion.  The modes and dipolar calls also run their finalize kernels (the palmer call stops at
the raw sums): kernel times alone come from running this script under `rocprofv3 --kernel-trace --stats`.  Per (j, lag) the modes kernel
issues 7 FMAs against 4 and 5, each from scalar windows.  No gate: the script reports."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from spinrelax_amd import synth                      # noqa: E402
from spinrelax_amd.hip import Context                # noqa: E402

PEAK_FP32 = 157.3e12                                 # MI355X vector FP32, FLOP/s (an FMA counts two)

s = synth.config_shapes(int(os.environ.get('CFG', '3')))
V = int(os.environ.get('NVEC', '512'))
R, F, L = s['R'], s['F'], s['F'] // 2
pre = synth.synth_vectors_parallel(s['frames'], V, s['seed'])
ctx = Context(0)
ctx.set_option('ct_fft', 0)                          # kernel 1 in its direct form: k_ct_palmer
vecs = torch.from_numpy(pre).cuda()
Npad = (s['frames'] + 63) // 64 * 64
soa = torch.empty((V, 3, Npad), device='cuda', dtype=torch.float32)
ctx.pack_soa_dev(vecs.data_ptr(), s['frames'], V, 0, V, soa.data_ptr(), Npad)
gen = torch.Generator(device='cuda').manual_seed(s['seed'])
dist = (0.3 * torch.exp(0.1 * torch.randn((s['frames'], V), device='cuda', generator=gen))).to(torch.float32)
soa4 = torch.empty((V, 4, Npad), device='cuda', dtype=torch.float32)
rref = torch.empty((V,), device='cuda', dtype=torch.float64)
ctx.pack_dipolar_dev(vecs.data_ptr(), dist.data_ptr(), s['frames'], V, 0, V, soa4.data_ptr(), Npad, rref.data_ptr())
soa5 = torch.empty((V, 5, Npad), device='cuda', dtype=torch.float32)
bad = torch.empty((V,), device='cuda', dtype=torch.int32)
q = np.array([0.4, -0.5, 0.3, 0.7])
ctx.pack_modes_dev(vecs.data_ptr(), s['frames'], V, 0, V, soa5.data_ptr(), Npad, bad.data_ptr(), frame=q / np.linalg.norm(q))
psum = torch.empty((6 * V * R * ctx.psum_stride(F),), device='cuda', dtype=torch.float64)
Ct = torch.empty((L, V), device='cuda', dtype=torch.float64)
dCt = torch.empty((L, V), device='cuda', dtype=torch.float64)
wm = torch.empty((V, 2), device='cuda', dtype=torch.float64)
H = torch.empty((L + 1, V, 6), device='cuda', dtype=torch.float64)
dH = torch.empty((L + 1, V, 6), device='cuda', dtype=torch.float64)
sm = torch.empty((V, 5), device='cuda', dtype=torch.float64)


def auto():
    ctx.ct_sums_dev(soa.data_ptr(), Npad, R, F, V, psum.data_ptr())


def dipolar():
    ctx.ct_dipolar_dev(soa4.data_ptr(), Npad, V, R, F, Ct.data_ptr(), dCt.data_ptr(), wm.data_ptr(), psum_ptr=psum.data_ptr())


def mode_sums():
    ctx.ct_modes_dev(soa5.data_ptr(), Npad, V, R, F, H.data_ptr(), dH.data_ptr(), sm.data_ptr(), psum_ptr=psum.data_ptr())


fns = (auto, dipolar, mode_sums)
for fn in fns:
    fn()
ctx.sync()
assert int(bad.sum().item()) == 0
ts = {fn: [] for fn in fns}
for _ in range(int(os.environ.get('REPS', '9'))):
    for fn in fns:
        ctx.timer_start()
        fn()
        ts[fn].append(ctx.timer_stop_ms())
trip = synth.exact_triples(R, F, V)                  # (j, lag) products, lags 1 .. L
flop = {auto: 8.0 * trip, dipolar: 10.0 * trip, mode_sums: 14.0 * trip}     # 4, 5 and 7 FMAs per product
ta = float(np.median(ts[auto]))
print('R=%d F=%d N=%d' % (R, F, V))
for fn, name in zip(fns, ('k_ct_palmer', 'ct_dipolar', 'ct_modes')):
    t = float(np.median(ts[fn]))
    print('  %-12s median %.3f ms (min %.3f)  %.1f TFLOP/s = %.1f %% of the FP32 vector peak   ratio to k_ct_palmer %.3f' %
          (name, t, min(ts[fn]), flop[fn] / t * 1e-9, 100.0 * flop[fn] / (t * 1e-3) / PEAK_FP32, t / ta))
print('  checksum %.12g' % float(H.sum().item()))
ctx.close()
