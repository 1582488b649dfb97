#!/usr/bin/env python3
"""Developer timing of k_ct_dipolar against k_ct_palmer (direct form, ct_fft = 0) on the same shape -- NVEC vectors (default 512) x the
chunks of cfg3 (24 x 4096 frames; CFG=2: cfg2's) --, alternating in one process on one device, device events around each call;
docs/EXPERIMENTS.md section 22.  The vectors are cfg3's unit vectors times a distance 0.3 exp(0.1 g), g standard normal.  The dipolar call
also runs k_ct_finalize and k_ct_dipolar_norm (the palmer call stops at the raw sums): kernel times alone come from running this script
under `rocprofv3 --kernel-trace --stats`.  Per (j, lag) the dipolar kernel issues 5 FMAs against 4 and per step 16 LDS reads against 12:
the counts give a ratio of 1.25 - 1.33; the gate is 1.5 (exit status 1 above it)."""
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
psum = torch.empty((V * R * ctx.psum_stride(F),), device='cuda', dtype=torch.float64)
Ct = torch.empty((L, V), device='cuda', dtype=torch.float64)
dCt = torch.empty((L, V), device='cuda', dtype=torch.float64)
wm = torch.empty((V, 2), device='cuda', dtype=torch.float64)


def auto():
    ctx.ct_sums_dev(soa.data_ptr(), Npad, R, F, V, psum.data_ptr())


def dipolar():
    ctx.ct_dipolar_dev(soa4.data_ptr(), Npad, V, R, F, Ct.data_ptr(), dCt.data_ptr(), wm.data_ptr(), psum_ptr=psum.data_ptr())


for fn in (auto, dipolar):
    fn()
ctx.sync()
ts = {auto: [], dipolar: []}
for _ in range(int(os.environ.get('REPS', '9'))):
    for fn in (auto, dipolar):
        ctx.timer_start()
        fn()
        ts[fn].append(ctx.timer_stop_ms())
ta, td = float(np.median(ts[auto])), float(np.median(ts[dipolar]))
trip = synth.exact_triples(R, F, V)                  # (j, lag) products, lags 1 .. L
fa, fd = 8.0 * trip, 10.0 * trip                     # 4 FMAs per product against 5
ratio = td / ta
print('R=%d F=%d N=%d  k_ct_palmer median %.3f ms (min %.3f) %.1f TFLOP/s = %.1f %% of the FP32 vector peak   ct_dipolar median %.3f ms '
      '(min %.3f) %.1f TFLOP/s = %.1f %%   ratio %.3f (gate %.2f)   checksum %.12g' %
      (R, F, V, ta, min(ts[auto]), fa / ta * 1e-9, 100.0 * fa / (ta * 1e-3) / PEAK_FP32, td, min(ts[dipolar]), fd / td * 1e-9,
       100.0 * fd / (td * 1e-3) / PEAK_FP32, ratio, GATE, float(Ct.sum().item())))
ctx.close()
sys.exit(0 if ratio <= GATE else 1)
