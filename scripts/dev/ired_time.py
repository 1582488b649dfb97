#!/usr/bin/env python3
"""Developer timing of the iRED matrix kernel pair (k_ired_matrix + k_ired_finish, sr_ired_matrix_f32_dev) alone at the cfg3 shape,
100 000 frames x 512 vectors, as one window and as 20 windows of 5 000 frames, against the obvious alternative on the same
device: materialise the (N, 6 F) float64 operand with torch (products of components, the weight 2 on the second operand) and
run one torch.matmul (batched over the windows); the materialisation is part of the alternative's time, since the kernel forms
its operands in registers.

Both are warmed up at every shape, timed with device events around REPS back-to-back calls (default 20), alternating, and the
two matrices are compared.  Useful work = 2 * 6 F * N (N + 1) / 2 flop per window (the upper triangle); the rate is given
against the FP64 vector peak that bench.py's roofline uses (78.6 TFLOP/s); the kernel executes 64 x 64 tiles, whole diagonal
tiles included, so it does T (T + 1) / 2 * 4096 / (N (N + 1) / 2) times as much (1.125 at N = 512).
KSPLIT=<s> forces the frame split, NVEC / FRAMES change the shape."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from spinrelax_amd.hip import Context                # noqa: E402

PEAK_FP64_TFLOPS = 78.6
N = int(os.environ.get('NVEC', '512'))
F = int(os.environ.get('FRAMES', '100000'))
REPS = int(os.environ.get('REPS', '20'))

ctx = Context(0)
if os.environ.get('KSPLIT'):
    ctx.set_option('ired_ksplit', int(os.environ['KSPLIT']))
g = torch.Generator(device='cuda').manual_seed(7)
vecs = torch.randn((F, N, 3), device='cuda', dtype=torch.float32, generator=g)
vecs /= vecs.norm(dim=-1, keepdim=True)
Npad = (F + 63) // 64 * 64
soa = torch.zeros((N, 3, Npad), device='cuda', dtype=torch.float32)
ctx.pack_soa_dev(vecs.data_ptr(), F, N, 0, N, soa.data_ptr(), Npad)
ctx.sync()
planes = soa[:, :, :F]


def ired(W, M):
    Fw = F // W
    ctx.ired_matrix_dev(soa.data_ptr(), Npad, N, np.arange(W) * Fw, np.full(W, Fw), M.data_ptr())


def alternative(W, M):
    Fw = F // W
    x, y, z = (planes[:, c, :W * Fw].double().reshape(N, W, Fw).permute(1, 0, 2) for c in range(3))       # (W, N, Fw) each
    A = torch.cat((x * x, y * y, z * z, x * y, x * z, y * z), dim=2)                                      # (W, N, 6 Fw)
    B = torch.cat((x * x, y * y, z * z, 2 * x * y, 2 * x * z, 2 * y * z), dim=2)
    torch.matmul(A, B.transpose(1, 2), out=M)
    M.mul_(1.5 / Fw).sub_(0.5)


def timed(fn, W, M):
    torch.cuda.synchronize()
    ctx.timer_start()
    for _ in range(REPS):
        fn(W, M)
    torch.cuda.synchronize()
    return ctx.timer_stop_ms() / REPS


for W in (1, 20):
    Ma = torch.empty((W, N, N), device='cuda', dtype=torch.float64)
    Mb = torch.empty((W, N, N), device='cuda', dtype=torch.float64)
    ired(W, Ma)
    alternative(W, Mb)
    torch.cuda.synchronize()
    diff = float((Ma - Mb).abs().max())
    ta, tb = [], []
    for _ in range(3):
        ta.append(timed(ired, W, Ma))
        tb.append(timed(alternative, W, Mb))
    flop = 2.0 * 6 * (F // W) * W * N * (N + 1) / 2
    t = min(ta)
    print('W=%2d  ired %.3f ms (runs %s)  torch materialise+matmul %.3f ms (runs %s)  max |dM| %.2e  useful %.1f TFLOP/s = %.1f %% of the FP64 '
          'vector peak' % (W, t, ' '.join('%.3f' % v for v in ta), min(tb), ' '.join('%.3f' % v for v in tb), diff, flop / t * 1e-9,
                           100.0 * flop / t * 1e-9 / PEAK_FP64_TFLOPS), flush=True)
ctx.close()
