#!/usr/bin/env python3
"""Developer timing of k_relax alone at cfg5 scale (4 096 residues x 9 experiments x 2 592 bins, weighted): the ellipsoid
(model 3) against the symmetric top (model 2) on the same device-resident inputs -- the launch the global Powell search pays
per objective evaluation.  Median of REPS (default 25) launches after warm-up, HIP events.  Prints a checksum of each table
so that variant builds (SPINRELAX_HIP_LIB) can be told apart from wrong ones; MODELS=2 times one model alone (a library
without model 3)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from spinrelax_amd import _hostmath as hm            # noqa: E402
from spinrelax_amd.hip import Context                # noqa: E402

n, B, Kmax = int(os.environ.get('NRES', '4096')), 2592, 8
fields = (500.0, 600.133, 800.0)
E = 3 * len(fields)
rng = np.random.default_rng(5)
gH, gN = 267.513e6, -27.116e6
om = np.zeros((E, 5))
for e in range(E):
    B0 = 2.0 * np.pi * fields[e // 3] / 267.513
    om[e, 1], om[e, 3] = -gN * B0 * 1e-12, -gH * B0 * 1e-12
    om[e, 2], om[e, 4] = om[e, 3] - om[e, 1], om[e, 3] + om[e, 1]
fdd = np.full(E, 0.10 * 1.1121216813552401e-82 * gN ** 2 * gH ** 2 * (1.02e-10) ** -6.0)
fcsa = np.array([np.repeat(2.0 / 15.0 * (-170e-6) ** 2 * (gN * 2.0 * np.pi * fields[e // 3] / 267.513) ** 2, n) for e in range(E)])
K = rng.integers(1, Kmax + 1, n).astype(np.int32)
C = rng.uniform(0.01, 0.04, (n, Kmax))
tau = 10.0 ** rng.uniform(0.5, 4.0, (n, Kmax))
S2 = 1.0 - C.sum(axis=1)
bv = hm.lambert_bin_vectors([np.linspace(-np.pi, np.pi, 73), np.linspace(-1.0, 1.0, 37)])
w = rng.poisson(3.0, (n, B)).astype(float)
Diso, aniso = 3.7e-5, 1.26
Dsym = list(hm.symmtop_from_iso(Diso, aniso))
Dell = list(hm.ellipsoid_from_iso(Diso, aniso, 0.4))

dev = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()      # noqa: E731
t = dict(om=dev(om), fdd=dev(fdd), fcsa=dev(fcsa), tf=dev(np.full(E, 1e-12)), gr=dev(np.full(E, gH / gN)), S2=dev(S2), C=dev(C),
         tau=dev(tau), K=dev(K, torch.int32), bv=dev(bv), w=dev(w))
out = torch.zeros((E, n, 4, 2), device='cuda', dtype=torch.float64)
stats = torch.zeros((E, n, 12), device='cuda', dtype=torch.float64)
ctx = Context(0)
reps = int(os.environ.get('REPS', '25'))
med = {}
for model, D in ((2, Dsym), (3, Dell)):
    if str(model) not in os.environ.get('MODELS', '2,3').split(','):
        continue

    def fn():
        ctx.relax_dev(model, D, E, t['om'].data_ptr(), t['fdd'].data_ptr(), t['fcsa'].data_ptr(), t['tf'].data_ptr(),
                      t['gr'].data_ptr(), n, Kmax, 0.89, t['S2'].data_ptr(), t['C'].data_ptr(), t['tau'].data_ptr(),
                      t['K'].data_ptr(), B, t['bv'].data_ptr(), t['w'].data_ptr(), 1, out.data_ptr(), None, stats.data_ptr())

    for _ in range(3):
        fn()
    ctx.sync()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop_ms())
    med[model] = float(np.median(ts))
    o = out.cpu().numpy()
    print('k_relax model %d  %d x %d x %d  median %.4f ms  min %.4f  max %.4f  (%d launches)  checksum %.17g'
          % (model, n, E, B, med[model], min(ts), max(ts), reps, float(o.sum())), flush=True)
    if os.environ.get('DUMP'):
        np.save(os.path.join(os.environ['DUMP'], 'relax_time_model%d.npy' % model), np.concatenate((o.ravel(), stats.cpu().numpy().ravel())))
if 2 in med and 3 in med:
    print('ratio model 3 / model 2: %.3f' % (med[3] / med[2]))
ctx.close()
