#!/usr/bin/env python3
"""Developer timing of the lagged dipolar map kernels (k_noe_lagged + k_noe_finish, sr_noe_lagged_f32_dev, mode 0, with
per-frame quaternions) against the map itself (k_noe_pairs + k_noe_finish, sr_noe_pairs_f32_dev) on the same coordinates in the same
run: 512 atoms x 100 000 frames as one block, one lag (K = 1, the lag LAG1, default 16) and twelve (noe.log_lags(2048, 12)).

All three are warmed up, and the lagged result is checked first: the lag computed alone has the bits it has in the list, and NCHECK
(default 64) pairs are recomputed in float64 by torch from the definition and compared relative to W = sum r(t)^-3 r(t + k)^-3.
A figure is device events around as many back-to-back calls as fill WINDOW_MS (default 500 ms; at least MIN_REPS = 3, the count
settled by one timed call), the three sides taking turns over ROUNDS (default 5) rounds; reported are the best, the median and the
worst round, per call, and for the lagged calls per lag and as a multiple of the map's time.  A call includes the upload of its
small tables with the stream synchronisation behind it, and the finish kernel.  The clocks are left as they are.
NATOMS / FRAMES / LAG1 / LAGMAX / LAGCOUNT change the shape."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from spinrelax_amd import noe                        # noqa: E402
from spinrelax_amd.hip import Context                # noqa: E402

WINDOW_MS = float(os.environ.get('WINDOW_MS', '500'))
MIN_REPS, ROUNDS = int(os.environ.get('MIN_REPS', '3')), int(os.environ.get('ROUNDS', '5'))
P, F = int(os.environ.get('NATOMS', '512')), int(os.environ.get('FRAMES', '100000'))
LAG1 = int(os.environ.get('LAG1', '16'))
LAGS = noe.log_lags(int(os.environ.get('LAGMAX', '2048')), int(os.environ.get('LAGCOUNT', '12')))
NCHECK = int(os.environ.get('NCHECK', '64'))

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


xyz, q = make(P, F)
index = np.arange(P)
npairs = P * (P - 1) // 2
bs, bl = [0], [F]
sums = torch.empty((1, npairs, 7), device=dev, dtype=torch.float64)
G1 = torch.empty((1, 1, npairs), device=dev, dtype=torch.float64)
GK = torch.empty((1, LAGS.size, npairs), device=dev, dtype=torch.float64)
torch.cuda.synchronize()
sides = [('k_noe_pairs', 0, lambda: ctx.noe_pairs_dev(xyz.data_ptr(), F, P, index, q.data_ptr(), bs, bl, sums.data_ptr(), mode=0)),
         ('k_noe_lagged K=1 (lag %d)' % LAG1, 1,
          lambda: ctx.noe_lagged_dev(xyz.data_ptr(), F, P, index, q.data_ptr(), bs, bl, [LAG1], G1.data_ptr(), mode=0)),
         ('k_noe_lagged K=%d (lags %s)' % (LAGS.size, ' '.join(str(k) for k in LAGS)), int(LAGS.size),
          lambda: ctx.noe_lagged_dev(xyz.data_ptr(), F, P, index, q.data_ptr(), bs, bl, LAGS, GK.data_ptr(), mode=0))]
for _, _, fn in sides:
    fn()
torch.cuda.synchronize()
ctx.sync()

# ---- the result, before any figure ----
if LAG1 in LAGS.tolist():
    same = torch.equal(G1[0, 0], GK[0, LAGS.tolist().index(LAG1)])
    print('lag %d alone and in the list of %d: %s' % (LAG1, LAGS.size, 'the same bits' if same else 'DIFFERENT BITS'))
pick = torch.from_numpy(np.random.default_rng(1).choice(npairs, size=min(NCHECK, npairs), replace=False)).to(dev)
pl = noe.pair_list(P)
iu, ju = torch.from_numpy(pl[:, 0]).to(dev)[pick], torch.from_numpy(pl[:, 1]).to(dev)[pick]
d = xyz[:, ju].double() - xyz[:, iu].double()
r = d.norm(dim=-1)
dp = torch.einsum('tab,tpb->tpa', rotmat(q), d)
worst = 0.0
for n, k in enumerate(LAGS.tolist()):
    a, c = slice(0, F - k), slice(k, F)
    ww = (r[a] * r[c]) ** -3
    cos2 = (dp[a] * dp[c]).sum(dim=-1) ** 2 / (r[a] * r[c]) ** 2
    ref = ((1.5 * cos2 - 0.5) * ww).sum(dim=0)
    worst = max(worst, float(((GK[0, n, pick] - ref).abs() / ww.sum(dim=0)).max()))
print('S = %d frame splits; %d pairs x %d lags against float64 torch: |G - ref| / W at most %.3g = %.2f u (bar 116 u)'
      % (ctx.noe_lagged_splits(P, F, 1), pick.numel(), LAGS.size, worst, worst * 2.0 ** 24))
del d, r, dp

# ---- the figures ----
reps = [max(MIN_REPS, int(np.ceil(WINDOW_MS / timed(fn, 1)))) for _, _, fn in sides]
t = [[] for _ in sides]
for _ in range(ROUNDS):
    for n, (_, _, fn) in enumerate(sides):
        t[n].append(timed(fn, reps[n]))
base = min(t[0])
for n, (name, K, _) in enumerate(sides):
    line = 'P=%d F=%d  %s: %s (%d rounds of %d calls)' % (P, F, name, fmt(t[n]), ROUNDS, reps[n])
    if K:
        line += '; per lag best %.3f ms = %.2f times k_noe_pairs; %.3g pair-frame-lags/s' % (
            min(t[n]) / K, min(t[n]) / K / base, float(npairs) * F * K / (min(t[n]) * 1e-3))
    else:
        line += '; %.3g pair-frames/s' % (float(npairs) * F / (min(t[n]) * 1e-3))
    print(line, flush=True)
ctx.close()
