#!/usr/bin/env python3
"""Developer timing of the iRED mode correlation functions (k_ired_project + k_ired_mode_ct, sr_ired_mode_ct_f32_dev) alone at the
cfg3 shape: 100 000 frames x 512 vectors, windows of 4096 frames (24 of them), K = 512 modes (a random orthogonal matrix per window),
n_lags = 2049, transform length 6144.

Warm-up, then device events around REPS back-to-back calls (default 20), best of three.  A call is two kernels per batch of
windows and the C ABI does not separate them: the per-kernel durations come from running this script under
`rocprofv3 --kernel-trace --stats` (REPS=3 is enough); the script prints the call's time and the flop counts the rates follow from.
Useful work: projection 2 * 6 * F_w * N * K flop per window, against the FP64 vector peak bench.py's roofline uses (78.6 TFLOP/s);
transforms 4 transforms of M points per (window, mode), 5 M log2 M flop each.
NVEC / FRAMES / WINDOW / NLAGS / WS_MB change the shape and the work area."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from spinrelax_amd.hip import Context                # noqa: E402

PEAK_FP64_TFLOPS = 78.6
N = int(os.environ.get('NVEC', '512'))
F = int(os.environ.get('FRAMES', '100000'))
Fw = int(os.environ.get('WINDOW', '4096'))
L = int(os.environ.get('NLAGS', str(Fw // 2 + 1)))
REPS = int(os.environ.get('REPS', '20'))
K = N
W = F // Fw

ctx = Context(0)
if os.environ.get('WS_MB'):
    ctx.set_option('ired_ws_mb', int(os.environ['WS_MB']))
g = torch.Generator(device='cuda').manual_seed(7)
vecs = torch.randn((F, N, 3), device='cuda', dtype=torch.float32, generator=g)
vecs /= vecs.norm(dim=-1, keepdim=True)
Npad = (F + 63) // 64 * 64
soa = torch.zeros((N, 3, Npad), device='cuda', dtype=torch.float32)
ctx.pack_soa_dev(vecs.data_ptr(), F, N, 0, N, soa.data_ptr(), Npad)
ctx.sync()
coef = torch.linalg.qr(torch.randn((W, N, N), device='cuda', dtype=torch.float64, generator=g))[0].contiguous()
Cm = torch.empty((W, K, L), device='cuda', dtype=torch.float64)
starts, lens = np.arange(W) * Fw, np.full(W, Fw)


def call():
    ctx.ired_mode_ct_dev(soa.data_ptr(), Npad, N, starts, lens, coef.data_ptr(), K, L, Cm.data_ptr())


def timed():
    torch.cuda.synchronize()
    ctx.timer_start()
    for _ in range(REPS):
        call()
    torch.cuda.synchronize()
    return ctx.timer_stop_ms() / REPS


call()
call()
torch.cuda.synchronize()
# spot check of one (window, mode, lag) against the definition in torch float64
w, m, k = W - 1, 3, 17
u = vecs[w * Fw:(w + 1) * Fw].double()
x, y, z = u[..., 0], u[..., 1], u[..., 2]
P = torch.stack((x * x, y * y, z * z, x * y, x * z, y * z), dim=-1)
A = torch.einsum('i,tic->tc', coef[w, m], P)
wts = torch.tensor([1.0, 1, 1, 2, 2, 2], device='cuda', dtype=torch.float64)
ref = 1.5 / (Fw - k) * float((A[:Fw - k] * A[k:] * wts).sum()) - 0.5 * float(coef[w, m].sum()) ** 2
print('check C[%d][%d][%d]: kernel %.15g definition %.15g' % (w, m, k, float(Cm[w, m, k]), ref), flush=True)
runs = [timed() for _ in range(3)]
t = min(runs)
need = Fw + L - 1
M = 2048 if need <= 2048 else 4096 if need <= 4096 else 6144 if need <= 6144 else 8192
flop_p = 2.0 * 6 * Fw * N * K * W
flop_t = 4.0 * 5 * M * np.log2(M) * W * K
print('W=%d windows of %d frames, N=K=%d, n_lags=%d, M=%d: call %.3f ms (runs %s); projection %.3e flop, transforms %.3e flop; if the '
      'projection were the whole call: %.1f TFLOP/s = %.1f %% of the FP64 vector peak'
      % (W, Fw, N, L, M, t, ' '.join('%.3f' % v for v in runs), flop_p, flop_t, flop_p / t * 1e-9, 100.0 * flop_p / t * 1e-9 / PEAK_FP64_TFLOPS),
      flush=True)
ctx.close()
