#!/usr/bin/env python3
"""Developer timing of the all-pairs dipolar map kernels (k_noe_pairs + k_noe_finish, sr_noe_pairs_f32_dev, mode 0, with per-frame
quaternions) alone at three shapes: 512 atoms x 100 000 frames as one block, the same frames as 24 blocks, and 128 atoms x 100 000
frames, against the same map from torch on the same device: broadcast differences of the selected atoms over chunks of frames small
enough to fit in memory (CHUNK frames, default 256: 256 x 130 816 pairs x 3 float32 = 0.4 GB per temporary), the rotation applied to
the difference vectors, the seven sums accumulated in float64.  The rotation matrices are formed once, outside the timed region.

Both are warmed up at every shape and the two results are compared.  A figure is device events around as many back-to-back calls
as fill WINDOW_MS (default 500 ms; at least MIN_REPS = 3, the count settled by one timed call), the two sides taking turns over
ROUNDS (default 5) rounds; reported are the best, the median and the worst round, per call.  A call of the kernel includes the
upload of its two small tables with the stream synchronisation behind it, and k_noe_finish.

Beside ms and pair-frames per second, two shares:
  of the FP32 vector ISSUE rate: the VALU instructions of the kernel's frame loop per thread (4 pairs) and frame, counted in the ISA
    (ISA below; profiles/README.md), each at what a SIMD with three waves issuing needs for it (COST, cycles; profiles/
    r05_pk_issue_rate.txt: a plain float32 instruction 2, v_pk_fma_f32 3.56, v_pk_mul / v_pk_add_f32 3.42; v_rsq_f32 twice a plain
    one; the float64 adds and conversions of the flush 4, profiles/r04_fp64_issue_rate.txt; moves 2), x pair-frames / 4 / 64 lanes,
    over 256 CUs x 4 SIMDs x CLOCK (default 2.4 GHz).  The time that sum alone would take is the lower bound of pure issue;
  of the FP32 vector peak (157.3 TFLOP/s, an fma counts two) at the 44 flop of a pair and frame, as ct_dipolar_time.py counts.
The kernel computes whole 32 x 32 tiles, three quarters of a diagonal one: 1.03 times the useful pairs at 512 atoms, 1.13 times at
128; both shares count the useful pairs only.
NATOMS / FRAMES / BLOCKS (comma lists of equal length) change the shapes."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from spinrelax_amd.hip import Context                # noqa: E402

WINDOW_MS = float(os.environ.get('WINDOW_MS', '500'))
MIN_REPS, ROUNDS = int(os.environ.get('MIN_REPS', '3')), int(os.environ.get('ROUNDS', '5'))
CHUNK = int(os.environ.get('CHUNK', '256'))
CLOCK = float(os.environ.get('CLOCK', '2.4e9'))
PEAK_FP32 = 157.3e12                                  # MI355X vector FP32, FLOP/s (an fma counts two)
FLOP = 44                                             # per pair and frame: 3 sub, 5 r2, 1 rsq, 4 powers, 15 rotation, 3 scale, 13 sums
# k_noe_pairs<float, true>, VALU instructions per thread (4 pairs): the frame loop, and the float64 flush that follows every 8th frame
ISA = dict(pk_fma=20, pk_mul_add=13, plain=50, rsq=4, mov_int=15)                # 102 per frame
ISA_FLUSH = dict(f64=56, mov=16)                                                  # 28 v_cvt_f64_f32, 28 v_add_f64; 13 v_mov_b64, 3 v_mov_b32
COST = dict(pk_fma=3.56, pk_mul_add=3.42, plain=2.0, rsq=4.0, mov_int=2.0, f64=4.0, mov=2.0)     # cycles of a SIMD, three waves issuing
CYCLES = sum(n * COST[k] for k, n in ISA.items()) + sum(n * COST[k] for k, n in ISA_FLUSH.items()) / 8.0      # per thread and frame
SIMD_CYCLES = 256 * 4 * CLOCK                         # per second, all SIMDs
NATOMS = [int(v) for v in os.environ.get('NATOMS', '512,512,128').split(',')]
FRAMES = [int(v) for v in os.environ.get('FRAMES', '100000,100000,100000').split(',')]
BLOCKS = [int(v) for v in os.environ.get('BLOCKS', '1,24,1').split(',')]

ctx = Context(0)
dev = torch.device('cuda', 0)


def make(P, F):
    """a jittered lattice of P points (spacing 0.4), tumbled and wobbling, 40 units from the origin; unit quaternions"""
    g = torch.Generator(device=dev).manual_seed(1000 * P + 1)
    n = int(np.ceil(P ** (1.0 / 3.0)))
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, device=dev)] * 3, indexing='ij'), dim=-1).reshape(-1, 3)[:P].float()
    body = 0.4 * grid + 0.1 * (torch.rand((P, 3), device=dev, generator=g) - 0.5)
    q = torch.randn((F, 4), device=dev, dtype=torch.float64, generator=g)
    q /= q.norm(dim=1, keepdim=True)
    xyz = body[None] + 0.02 * torch.randn((F, P, 3), device=dev, generator=g) + 40.0
    return xyz.contiguous(), q.contiguous()


def rotmat(q):
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                        2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def kernel(xyz, q, index, bs, bl, out, _R, _iu, _ju):
    ctx.noe_pairs_dev(xyz.data_ptr(), xyz.shape[0], xyz.shape[1], index, q.data_ptr(), bs, bl, out.data_ptr(), mode=0)


def alternative(xyz, q, index, bs, bl, out, R, iu, ju):
    out.zero_()
    for b in range(len(bs)):
        for s in range(bs[b], bs[b] + bl[b], CHUNK):
            e = min(s + CHUNK, bs[b] + bl[b])
            x = xyz[s:e]
            d = x[:, ju] - x[:, iu]                                        # (chunk, pairs, 3)
            r2 = (d * d).sum(dim=-1)
            ri = torch.rsqrt(r2)
            ri3 = ri * ri * ri
            dp = torch.einsum('tab,tpb->tpa', R[s:e], d)
            sc = dp * (ri3 * ri * ri)[..., None]
            out[b, :, 0] += (ri3 * ri3).double().sum(dim=0)
            out[b, :, 1:4] += (sc * dp).double().sum(dim=0)
            out[b, :, 4] += (sc[..., 0] * dp[..., 1]).double().sum(dim=0)
            out[b, :, 5] += (sc[..., 0] * dp[..., 2]).double().sum(dim=0)
            out[b, :, 6] += (sc[..., 1] * dp[..., 2]).double().sum(dim=0)


def timed(fn, args, reps):
    torch.cuda.synchronize()
    ctx.timer_start()
    for _ in range(reps):
        fn(*args)
    torch.cuda.synchronize()
    ctx.sync()
    return ctx.timer_stop_ms() / reps


def fmt(t):
    return 'best %.3f median %.3f worst %.3f ms' % (min(t), float(np.median(t)), max(t))


for P, F, B in zip(NATOMS, FRAMES, BLOCKS):
    xyz, q = make(P, F)
    R = rotmat(q).float()
    index = np.arange(P)
    iu, ju = (torch.from_numpy(a).to(dev) for a in np.triu_indices(P, k=1))
    Fb = F // B
    bs, bl = [b * Fb for b in range(B)], [Fb] * B
    npairs = P * (P - 1) // 2
    a = torch.empty((B, npairs, 7), device=dev, dtype=torch.float64)
    b = torch.empty((B, npairs, 7), device=dev, dtype=torch.float64)
    args = (xyz, q, index, bs, bl)
    kernel(*args, a, R, iu, ju)
    alternative(*args, b, R, iu, ju)
    torch.cuda.synchronize()
    ctx.sync()
    d6 = float((a[..., 0] / b[..., 0] - 1).abs().max())
    dt = float(((a[..., 1:] - b[..., 1:]).abs() / (b[..., 1] + b[..., 2] + b[..., 3])[..., None]).max())
    ra = max(MIN_REPS, int(np.ceil(WINDOW_MS / timed(kernel, args + (a, R, iu, ju), 1))))
    rb = max(MIN_REPS, int(np.ceil(WINDOW_MS / timed(alternative, args + (b, R, iu, ju), 1))))
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(timed(kernel, args + (a, R, iu, ju), ra))
        tb.append(timed(alternative, args + (b, R, iu, ju), rb))
    pf = float(npairs) * Fb * B
    t = min(ta)
    issue_ms = pf / 4.0 / 64.0 * CYCLES / SIMD_CYCLES * 1e3
    print('P=%d F=%d B=%d  noe %s (%d rounds of %d calls)  torch broadcast %s (of %d calls)  r^-6 sums rel %.2e, tensor / sum r^-3 %.2e  '
          '%.3g pair-frames/s; pure issue at %.1f cycles per thread and frame %.2f ms = %.1f %% of the time; %.1f TFLOP/s = %.1f %% of '
          'the FP32 vector peak'
          % (P, F, B, fmt(ta), ROUNDS, ra, fmt(tb), rb, d6, dt, pf / t * 1e3, CYCLES, issue_ms, 100.0 * issue_ms / t,
             pf * FLOP / (t * 1e-3) * 1e-12, 100.0 * pf * FLOP / (t * 1e-3) / PEAK_FP32), flush=True)
ctx.close()
