#!/usr/bin/env python3
"""Developer tool: one sha256 per case of the raw output arrays of Context.noe_pairs, noe_lagged and noe_modes from seeded inputs, to
compare two builds of the library bit by bit:

    SPINRELAX_HIP_LIB=/path/to/other/libspinrelax_hip.so scripts/dev/noe_bits.py > a.txt
    scripts/dev/noe_bits.py > b.txt && cmp a.txt b.txt

Cases, for each of the three calls: both modes; with and without per-frame quaternions (noe_modes also with the frame quaternion alone);
P = 2, 33 and 65 atoms over 120 frames as the ragged blocks (0, 37), (37, 20), (60, 40); P = 5 over 300 frames, where two frame
splits and the finish kernel run (asserted); for the map, P = 67 over 1000 frames as 1 and as 3 blocks (splits, asserted).  The
digests depend on the compiler as well as on the source: a record of one comparison, not a golden file."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from spinrelax_amd.hip import Context                # noqa: E402

ctx = Context(0)


def make(P, F, seed):
    """P selected atoms of P + 3, a jittered lattice of spacing 0.4 that wobbles, far from the origin; unit quaternions"""
    rng = np.random.default_rng(seed)
    nA = P + 3
    n = int(np.ceil(nA ** (1.0 / 3.0)))
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing='ij'), axis=-1).reshape(-1, 3)[:nA]
    body = 0.4 * grid + 0.1 * (rng.random((nA, 3)) - 0.5)
    xyz = (body[None] + 0.03 * rng.standard_normal((F, nA, 3)) + 40.0).astype(np.float32)
    q = rng.standard_normal((F, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return xyz, q, rng.permutation(nA)[:P].astype(np.int32)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


FRAME = np.array([0.5, -0.1, 0.7, 0.5])
FRAME /= np.linalg.norm(FRAME)
RAGGED = ([0, 37, 60], [37, 20, 40])
SHAPES = [(P, 120, RAGGED, [0, 1, 7, 19]) for P in (2, 33, 65)] + [(5, 300, (None, None), [0, 3, 129])]
assert ctx.noe_lagged_splits(5, 300, 1) == 2
assert ctx.noe_lagged_splits(67, 1000, 1) > 1 and ctx.noe_lagged_splits(67, 333, 3) > 1

for P, F, (bs, bl), lags in SHAPES:
    xyz, q, index = make(P, F, 100 * P + F)
    for mode in (0, 1):
        for quat in (None, q):
            tag = 'P=%d F=%d B=%d mode=%d quat=%d' % (P, F, 1 if bs is None else len(bs), mode, quat is not None)
            print('noe_pairs  %s  %s' % (tag, digest(ctx.noe_pairs(xyz, index, quat=quat, block_start=bs, block_len=bl, mode=mode))))
            print('noe_lagged %s  %s' % (tag, digest(ctx.noe_lagged(xyz, index, lags, quat=quat, block_start=bs, block_len=bl, mode=mode))))
            for frame in (None, FRAME):
                print('noe_modes  %s frame=%d  %s' % (tag, frame is not None, digest(
                    ctx.noe_modes(xyz, index, lags, quat=quat, frame=frame, block_start=bs, block_len=bl, mode=mode))))
xyz, q, index = make(67, 1000, 67)
for bs, bl in ((None, None), ([0, 333, 666], [333, 333, 334])):
    for mode in (0, 1):
        for quat in (None, q):
            print('noe_pairs  P=67 F=1000 B=%d mode=%d quat=%d  %s' % (1 if bs is None else 3, mode, quat is not None, digest(
                ctx.noe_pairs(xyz, index, quat=quat, block_start=bs, block_len=bl, mode=mode))))
ctx.close()
