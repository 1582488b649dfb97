#!/usr/bin/env python3
"""Developer timing of the NOESY kernels (csrc/sr_noesy.hip) at P = 512, 1024 and 4096 spins (P, a comma list, changes the shapes):

  product      k_symm_mul + k_symm_mul_finish (sr_symm_mul_f64_dev) on a random symmetric A and B = I + A / 2 + A A / 4, against
               torch.matmul of the same float64 operands on the same device in the same run;
  exponential  the whole sr_symm_expm_f64_dev for one mixing time of 0.2 s (the row sums, their copy to the host, the Horner products
               and the squarings) on a synthetic rate matrix scaled to |R|_1 = NORM1 (default 110 / s, what a protein at tau_c = 5 ns
               gives: s = 6 at 0.2 s), against torch.linalg.matrix_exp of -0.2 R on the device.

Both sides are warmed up at every shape and their results compared.  A figure is device events around as many back-to-back calls as
fill WINDOW_MS (default 300 ms; at least MIN_REPS = 3, the count settled by one timed call), the two sides taking turns over ROUNDS
(default 5) rounds; reported are the best, the median and the worst round, per call.  The clocks are not touched.

The share of the FP64 matrix peak (78.6 TFLOP/s) counts the flops of the tiles actually computed: T (T + 1) / 2 tiles of 64 x 64,
T = ceil(P / 64), each 2 x 64 x 64 x P -- about half of a general product's 2 P^3."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from spinrelax_amd import hip                        # noqa: E402

WINDOW_MS = float(os.environ.get('WINDOW_MS', '300'))
MIN_REPS, ROUNDS = int(os.environ.get('MIN_REPS', '3')), int(os.environ.get('ROUNDS', '5'))
PEAK_FP64_MATRIX = 78.6e12
NORM1 = float(os.environ.get('NORM1', '110'))
TAU = 0.2
SHAPES = [int(v) for v in os.environ.get('P', '512,1024,4096').split(',')]

ctx = hip.Context(0)
dev = torch.device('cuda', 0)


def timed(fn, reps):
    torch.cuda.synchronize()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ctx.sync()
    return ctx.timer_stop_ms() / reps


def fmt(t):
    return 'best %.3f median %.3f worst %.3f ms' % (min(t), float(np.median(t)), max(t))


def race(a, b):
    a(); b()
    torch.cuda.synchronize()
    ctx.sync()
    ra = max(MIN_REPS, int(np.ceil(WINDOW_MS / timed(a, 1))))
    rb = max(MIN_REPS, int(np.ceil(WINDOW_MS / timed(b, 1))))
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(timed(a, ra))
        tb.append(timed(b, rb))
    return ta, tb, ra, rb


for P in SHAPES:
    g = torch.Generator(device=dev).manual_seed(P)
    A = torch.randn((P, P), device=dev, dtype=torch.float64, generator=g) / np.sqrt(P)
    A = (A + A.T).contiguous()
    B = (torch.eye(P, device=dev, dtype=torch.float64) + A / 2 + (A @ A) / 4)
    B = ((B + B.T) / 2).contiguous()
    C, Ct = torch.empty_like(A), torch.empty_like(A)
    T = (P + 63) // 64
    flop = T * (T + 1) // 2 * 2.0 * 64 * 64 * P

    def mine():
        ctx.symm_mul_dev(A.data_ptr(), B.data_ptr(), P, C.data_ptr())

    def theirs():
        torch.matmul(A, B, out=Ct)

    ta, tb, ra, rb = race(mine, theirs)
    diff = float((C - Ct).abs().max())
    t = min(ta)
    print('P=%d product  k_symm_mul %s (%d rounds of %d calls)  torch.matmul %s (of %d calls)  ratio of the best %.2f  max |diff| %.2e  '
          '%.2f TFLOP/s on the computed tiles = %.1f %% of the FP64 matrix peak'
          % (P, fmt(ta), ROUNDS, ra, fmt(tb), rb, min(ta) / min(tb), diff, flop / (t * 1e-3) * 1e-12, 100.0 * flop / (t * 1e-3) / PEAK_FP64_MATRIX),
          flush=True)

    # a rate matrix of the usual structure: negative off-diagonal elements falling off with the index distance, a dominant diagonal
    i = torch.arange(P, device=dev, dtype=torch.float64)
    R = -1.0 / (1.0 + (i[:, None] - i[None, :]).abs()) ** 2
    R.fill_diagonal_(0.0)
    R = R - torch.diag(R.sum(dim=1)) * 1.2
    R = (R * (NORM1 / float(R.abs().sum(dim=1).max()))).contiguous()
    s, products = hip.symm_expm_plan(float(R.abs().sum(dim=1).max()), TAU)
    E = torch.empty((1, P, P), device=dev, dtype=torch.float64)
    Et = [None]

    def mine_e():
        ctx.symm_expm_dev(R.data_ptr(), P, [TAU], E.data_ptr())

    def theirs_e():
        Et[0] = torch.linalg.matrix_exp(-TAU * R)

    ta, tb, ra, rb = race(mine_e, theirs_e)
    diff = float((E[0] - Et[0]).abs().max())
    t = min(ta)
    print('P=%d exponential (s = %d, %d products)  symm_expm %s (%d rounds of %d calls)  torch.linalg.matrix_exp %s (of %d calls)  ratio of '
          'the best %.2f  max |diff| %.2e  %.2f TFLOP/s on the computed tiles = %.1f %% of the FP64 matrix peak'
          % (P, s, products, fmt(ta), ROUNDS, ra, fmt(tb), rb, min(ta) / min(tb), diff, products * flop / (t * 1e-3) * 1e-12,
             100.0 * products * flop / (t * 1e-3) / PEAK_FP64_MATRIX), flush=True)
ctx.close()
