"""
Host-side mirror of the C(t) / vector-distribution functions of the reference's
calculate-Ct-from-traj.py, with the same names, argument meaning and error behaviour, computing on the
MI355X through libspinrelax_hip.so.  There is no CPU compute path here: index arithmetic and
formatting only; the arithmetic of the hot loops runs in the HIP kernels.
"""
import sys

import numpy as np

from . import hip
from . import dist as srdist


def _ctx(ctx):
    return ctx if ctx is not None else hip.default_context()


def calculate_dt(dt, tau):
    """calculate-Ct-from-traj.py:240-243: the lag axis (arange(int(0.5*tau/dt)) + 1) * dt."""
    nPts = int(0.5 * tau / dt)
    return (np.arange(nPts) + 1.0) * dt


def concat_with_chunk_starts(vec_list, F):
    """Index form of reformat_vecs_by_tau (calculate-Ct-from-traj.py:245-275): instead of copying the
    used frames into a (R, F, V, 3) array, return the concatenation of the files, the start frame of
    each of the R chunks and R.  The tail of every file that does not fill a chunk is skipped."""
    starts = []
    off = 0
    for v in vec_list:
        n = v.shape[0]
        for c in range(n // F):
            starts.append(off + c * F)
        off += n
    cat = vec_list[0] if len(vec_list) == 1 else np.concatenate(vec_list, axis=0)
    return np.ascontiguousarray(cat, dtype=np.float32), np.array(starts, dtype=np.int64), len(starts)


def reformat_vecs_by_tau(vecs, dt, tau):
    """calculate-Ct-from-traj.py:245-275, same signature and prints: list of (frames, bonds, 3) arrays ->
    (nchunk, frames_per_chunk, bonds, 3).  Kept for callers that want the 4-D array; the GPU path itself
    uses concat_with_chunk_starts and never materialises it."""
    nFiles = len(vecs)
    nFramesPerChunk = int(tau / dt)
    print("    ...debug: Using %i frames per chunk based on tau/dt (%g/%g)." % (nFramesPerChunk, tau, dt))
    kept = []
    for i in range(nFiles):
        nFrames = vecs[i].shape[0]
        used = int(nFrames / nFramesPerChunk) * nFramesPerChunk
        print("    ...Source %i divided into %i chunks. Usage rate: %g %%" % (i, used / nFramesPerChunk, 100.0 * used / nFrames))
        kept.append(vecs[i][0:used, ...])
    out = np.concatenate(kept, axis=0)
    nTot = out.shape[0]
    print("    ...Done. vecs reformatted into %i chunks." % (nTot / nFramesPerChunk))
    return out.reshape((int(nTot / nFramesPerChunk), nFramesPerChunk, out.shape[-2], out.shape[-1]))


def calculate_Ct_Palmer(vecs, ctx=None, mode=0, v0=0, nV=None):
    """calculate-Ct-from-traj.py:200-238.  vecs (nReplicates, nFrames, nResidues, 3) -> Ct, dCt of shape
    (nDeltas, nResidues), float64 (the reference returns the dtype of vecs; the values here are the
    float64 evaluation, see DESIGN.md "precision")."""
    sh = vecs.shape
    print("= = = Debug of calculate_Ct_Palmer confirming the dimensions of vecs:", sh)
    if len(sh) != 4:
        print("= = = ERROR: The input vectors to calculate_Ct_Palmer is not of the expected 4-dimensional form! ", sh,
              file=sys.stderr)
        sys.exit(1)
    if sh[1] < 50:
        print("= = = WARNING: there are less than 50 frames per block of memory-time!", file=sys.stderr)
    R, F, V = sh[0], sh[1], sh[2]
    flat = np.ascontiguousarray(vecs, dtype=np.float32).reshape(R * F, V, 3)
    return _ctx(ctx).ct_palmer(flat, R, F, v0=v0, nV=nV, mode=mode)


def calculate_Ct_from_files(vec_list, dt, tau, ctx=None, mode=0, v0=0, nV=None):
    """reformat_vecs_by_tau + calculate_Ct_Palmer without the intermediate copy."""
    F = int(tau / dt)
    cat, starts, R = concat_with_chunk_starts(vec_list, F)
    if R < 1:
        print("= = = ERROR: no trajectory holds a full block of memory time tau!", file=sys.stderr)
        sys.exit(1)
    if srdist.world() > 1 and nV is None and v0 == 0:
        # several ranks (torchrun): vectors are independent -- every rank computes its contiguous range of columns, all
        # ranks receive the whole (lags, vectors) arrays
        V = cat.shape[1]
        i0, nloc = srdist.my_range(V)
        L = F // 2
        if nloc > 0:
            Ct, dCt = _ctx(ctx).ct_palmer(cat, R, F, v0=i0, nV=nloc, chunk_start=starts, mode=mode)
        else:
            Ct, dCt = np.empty((L, 0)), np.empty((L, 0))
        return srdist.gather_rows(Ct, V, axis=1), srdist.gather_rows(dCt, V, axis=1)
    return _ctx(ctx).ct_palmer(cat, R, F, v0=v0, nV=nV, chunk_start=starts, mode=mode)


def read_pairs(path, nV):
    """The pair file of --crossCt: one pair per line, two integers, indices into the list of nV vectors (0-based); blank lines and
    everything behind a '#' are ignored.  Returns an (nP, 2) int32 array.  Pure parsing: a malformed line, an index outside
    [0, nV) and a file without pairs raise ValueError, before any device call."""
    pairs = []
    with open(path) as fp:
        for n, line in enumerate(fp, 1):
            tok = line.split('#', 1)[0].split()
            if not tok:
                continue
            try:
                if len(tok) != 2:
                    raise ValueError
                i, j = int(tok[0]), int(tok[1])
            except ValueError:
                raise ValueError('%s line %d: expected two integers, got %r' % (path, n, line.rstrip('\n'))) from None
            if not (0 <= i < nV and 0 <= j < nV):
                raise ValueError('%s line %d: pair (%d, %d) is outside the %d vectors (indices are 0 .. %d)' % (path, n, i, j, nV, nV - 1))
            pairs.append((i, j))
    if not pairs:
        raise ValueError('%s holds no pairs' % path)
    return np.array(pairs, dtype=np.int32)


def _check_pairs(pairs, nV):
    """shape, type and range of a pair table, before any device call"""
    return np.stack(hip.pair_columns(pairs, nV), axis=1)


def _dispatch(rv, stem, label, F, *args, **kw):
    """The dispatch of the three extensions of C(t), stem = 'cross', 'dipolar' or 'dipolar_cross': chunks that the staged kernel can hold
    go to it (rv.ct_<stem>), longer ones -- and, under sr_set_option("ct_<stem>_long_min_frames", n), every chunk of at least n frames --
    to the blocked form (rv.ct_<stem>_long); args and kw are handed on to either."""
    c = rv.ctx
    direct_max = getattr(c, 'ct_%s_max_frames' % stem)()
    long_max = getattr(c, 'ct_%s_long_max_frames' % stem)()
    if F > long_max:
        raise ValueError('%s: a chunk of %d frames is beyond both forms (the staged kernel takes %d frames, the blocked transforms %d)'
                         % (label, F, direct_max, long_max))
    blocked = F > direct_max or F >= getattr(c, 'ct_%s_long_min_frames' % stem)
    return getattr(rv, 'ct_%s_long' % stem if blocked else 'ct_%s' % stem)(*args, **kw)


def _ct_cross(rv, R, F, pairs, **kw):
    return _dispatch(rv, 'cross', 'cross-correlation functions', F, R, F, pairs, **kw)


def calculate_Ct_cross(vecs, pairs, symmetric=True, ctx=None, mode=0):
    """Time-lagged P2 cross-correlation functions between pairs of vectors, C_ij(k) = <P2(u_i(t) . u_j(t + k))>, an extension beyond
    the reference.  vecs (nReplicates, nFrames, nVectors, 3) as calculate_Ct_Palmer takes them, pairs (nP, 2) indices into the vectors.
    Returns P0 (nP), the equal-time value <P2(u_i . u_j)>, and Ct, dCt (nFrames // 2, nP) for the lags 1 .. nFrames // 2: mean over
    the replicates and std / (sqrt(nReplicates) - 1) like C(t).  symmetric (the default): (C_ij + C_ji) / 2, the function relaxation
    theory uses, equal to the autocorrelation for i = j; otherwise C_ij alone, the later frame taken from vector j."""
    sh = np.shape(vecs)
    if len(sh) != 4 or sh[3] != 3:
        raise ValueError('vecs must be (replicates, frames, vectors, 3), got %s' % (sh,))
    R, F, V = sh[0], sh[1], sh[2]
    pairs = _check_pairs(pairs, V)
    flat = np.ascontiguousarray(vecs, dtype=np.float32).reshape(R * F, V, 3)
    with _ctx(ctx).vectors(V, R * F) as rv:
        rv.append(flat)
        return _ct_cross(rv, R, F, pairs, sym=int(bool(symmetric)), mode=mode)


def calculate_Ct_cross_from_files(vec_list, dt, tau, pairs, symmetric=True, ctx=None, mode=0):
    """calculate_Ct_cross on the chunks reformat_vecs_by_tau would form from the files (concat_with_chunk_starts: the tail of every
    file that does not fill a chunk of int(tau / dt) frames is skipped, exactly as for C(t))."""
    F = int(tau / dt)
    cat, starts, R = concat_with_chunk_starts(vec_list, F)
    if R < 1:
        raise ValueError('no trajectory holds a full block of memory time tau')
    pairs = _check_pairs(pairs, cat.shape[1])
    with _ctx(ctx).vectors(cat.shape[1], cat.shape[0]) as rv:
        rv.append(cat)
        return _ct_cross(rv, R, F, pairs, chunk_start=starts, sym=int(bool(symmetric)), mode=mode)


def calculate_Ct_cross_resident(rv, pairs, R, F, symmetric=True, mode=0, chunk_start=None, want_dP0=False):
    """calculate_Ct_cross of resident vectors (regular chunks r * F unless chunk_start is given).  A pair needs both of its vectors on
    one GPU: rv holds ALL vectors (a single process), not a rank's range.  want_dP0: (P0, dP0, Ct, dCt), dP0 the error of P0 over the
    chunks, std / (sqrt(R) - 1) like dCt."""
    pairs = _check_pairs(pairs, rv.nV)
    return _ct_cross(rv, R, F, pairs, chunk_start=chunk_start, sym=int(bool(symmetric)), mode=mode, want_dP0=want_dP0)


def _check_dist(dist, shape):
    """shape and values of a distance array, before any device call: float32 (what the library takes), positive and finite"""
    d = np.ascontiguousarray(dist, dtype=np.float32)
    if d.shape != tuple(shape):
        raise ValueError('dist must have the shape %s of the vectors without their last axis, got %s' % (tuple(shape), d.shape))
    if not (np.all(np.isfinite(d)) and np.all(d > 0)):
        raise ValueError('dist holds an entry that is not positive and finite')
    return d


def _ct_dipolar(rv, R, F, **kw):
    return _dispatch(rv, 'dipolar', 'dipolar correlation function', F, R, F, **kw)


def _ct_dipolar_cross(rv, R, F, pairs, **kw):
    return _dispatch(rv, 'dipolar_cross', 'dipolar cross-correlation functions', F, R, F, pairs, **kw)


def calculate_Ct_dipolar(vecs, dist=None, ctx=None, mode=0):
    """Distance-weighted dipolar correlation function of flexible spin pairs, an extension beyond the reference:
    C_dd(k) = <P2(u(t) . u(t + k)) r(t)^-3 r(t + k)^-3> / <r^-6> (Brueschweiler et al. 1992; Peter, Daura & van Gunsteren 2001).
    vecs (nReplicates, nFrames, nVectors, 3) as calculate_Ct_Palmer takes them, but of any length: the length of a vector is the
    distance r, unless dist (nReplicates, nFrames, nVectors) gives it -- then the vectors only give the direction.
    Returns (Ct, dCt, reff6, reff3, S2rad): Ct, dCt (nFrames // 2, nVectors) for the lags 1 .. nFrames // 2, the ratio of the mean over
    the replicates of the unnormalised function to the mean of its lag-0 value, and std / (sqrt(nReplicates) - 1) of the former over
    the same normaliser (whose own scatter is ignored); per vector the effective distances reff6 = <r^-6>^(-1/6), reff3 = <r^-3>^(-1/3)
    and the radial order parameter S2rad = <r^-3>^2 / <r^-6>, over all frames, in the units of the input.  Replicates longer than
    Context.ct_dipolar_max_frames() frames take the blocked form, up to Context.ct_dipolar_long_max_frames() frames (_ct_dipolar)."""
    sh = np.shape(vecs)
    if len(sh) != 4 or sh[3] != 3:
        raise ValueError('vecs must be (replicates, frames, vectors, 3), got %s' % (sh,))
    R, F, V = sh[0], sh[1], sh[2]
    if dist is not None:
        dist = _check_dist(dist, (R, F, V)).reshape(R * F, V)
    flat = np.ascontiguousarray(vecs, dtype=np.float32).reshape(R * F, V, 3)
    with _ctx(ctx).vectors(V, R * F) as rv:
        rv.append(flat)
        return _ct_dipolar(rv, R, F, dist=dist, mode=mode)


def calculate_Ct_dipolar_resident(rv, R, F, dist=None, mode=0, chunk_start=None):
    """calculate_Ct_dipolar of resident vectors (regular chunks r * F unless chunk_start is given); dist (frames held, vectors).  r_ref is
    the shortest distance among all frames held; the averages behind reff6, reff3 and S2rad run over the frames of the chunks used."""
    if dist is not None:
        dist = _check_dist(dist, (rv.frames, rv.nV))
    return _ct_dipolar(rv, R, F, dist=dist, chunk_start=chunk_start, mode=mode)


def calculate_Ct_dipolar_cross(vecs, pairs, dist=None, symmetric=True, ctx=None, mode=0):
    """Distance-weighted P2 cross-correlation functions between pairs of flexible spin pairs, the function of dipole-dipole
    cross-correlated relaxation, an extension beyond the reference:
    C_ij(k) = <P2(u_i(t) . u_j(t + k)) r_i(t)^-3 r_j(t + k)^-3> / sqrt(<r_i^-6> <r_j^-6>).
    vecs and dist as calculate_Ct_dipolar takes them, pairs (nP, 2) and symmetric as calculate_Ct_cross.  Returns
    (P0, dP0, Ct, dCt, reff6): the equal-time value and its error over the replicates (nP), Ct, dCt (nFrames // 2, nP) for the lags
    1 .. nFrames // 2 -- ratios of the replicate means to sqrt(n_i n_j), n_v the replicate mean of <w_v^2>, whose own scatter is
    ignored -- and reff6 (nP, 2), the effective distances <r^-6>^(-1/6) of the two vectors of each pair.  For i = j: C_dd of
    calculate_Ct_dipolar and P0 = 1.  Replicates longer than Context.ct_dipolar_cross_max_frames() frames take the blocked form, up to
    Context.ct_dipolar_cross_long_max_frames() frames (_ct_dipolar_cross)."""
    sh = np.shape(vecs)
    if len(sh) != 4 or sh[3] != 3:
        raise ValueError('vecs must be (replicates, frames, vectors, 3), got %s' % (sh,))
    R, F, V = sh[0], sh[1], sh[2]
    pairs = _check_pairs(pairs, V)
    if dist is not None:
        dist = _check_dist(dist, (R, F, V)).reshape(R * F, V)
    flat = np.ascontiguousarray(vecs, dtype=np.float32).reshape(R * F, V, 3)
    with _ctx(ctx).vectors(V, R * F) as rv:
        rv.append(flat)
        return _ct_dipolar_cross(rv, R, F, pairs, dist=dist, sym=int(bool(symmetric)), mode=mode)


def calculate_Ct_dipolar_cross_resident(rv, pairs, R, F, dist=None, symmetric=True, mode=0, chunk_start=None):
    """calculate_Ct_dipolar_cross of resident vectors (regular chunks r * F unless chunk_start is given); dist (frames held, vectors).  rv
    holds ALL vectors (a single process).  r_ref is the shortest distance among all frames held; the averages behind reff6 run over the
    frames of the chunks used."""
    pairs = _check_pairs(pairs, rv.nV)
    if dist is not None:
        dist = _check_dist(dist, (rv.frames, rv.nV))
    return _ct_dipolar_cross(rv, R, F, pairs, dist=dist, chunk_start=chunk_start, sym=int(bool(symmetric)), mode=mode)


def _modes_result(rv, R, F, frame, chunk_start, mode):
    """the dict of the three calculate_Ct_modes functions; a chunk beyond the staged kernel raises before any device work"""
    from .noe import _frame_quat
    q = _frame_quat(frame)
    fmax = rv.ctx.ct_modes_max_frames()
    if F > fmax:
        raise ValueError('mode-resolved C(t): a chunk of %d frames is beyond the staged kernel (%d frames), the only form of this function'
                         % (F, fmax))
    H, dH, smean = rv.ct_modes(R, F, frame=q, chunk_start=chunk_start, mode=mode)
    return dict(H=H, dH=dH, smean=smean, frame=np.array([1.0, 0.0, 0.0, 0.0]) if q is None else q, lags=np.arange(F // 2 + 1))


def calculate_Ct_modes(vecs, frame=None, ctx=None, mode=0):
    """The bond-vector correlation function split into the five tumbling modes of an anisotropic diffusion tensor, an extension beyond
    the reference (whose anisotropic J(w) multiplies a static orientation histogram by one internal C(t)).  vecs (nReplicates, nFrames,
    nVectors, 3) as calculate_Ct_Palmer takes them, of any positive length; frame: the unit quaternion (w, x, y, z) that rotates them
    into the principal-axis frame of the tensor, --vecRot's convention (noe.frame_matrix), or None.  With u the rotated unit vector,
    s0 = u_z^2 - 1/3, s1 = u_x^2 - u_y^2, s2 = u_y u_z, s3 = u_x u_z, s4 = u_x u_y and s' the signal k frames later, returns a dict:
    H, dH (nFrames // 2 + 1, nVectors, 6) = <s0 s0'>, <s1 s1'>, <s0 s1' + s1 s0'> / 2, <s2 s2'>, <s3 s3'>, <s4 s4'> at the lags
    0 .. nFrames // 2 (the order of noe.mode_amplitudes), mean over the replicates and std / (sqrt(nReplicates) - 1) like C(t);
    smean (nVectors, 5), the means of the five signals over all frames; frame (the quaternion, (1, 0, 0, 0) for None) and lags.
    They do not depend on the tensor: modes.amplitudes, modes.J and modes.relaxation take this dict and any D.  Replicates of up to
    Context.ct_modes_max_frames() frames."""
    sh = np.shape(vecs)
    if len(sh) != 4 or sh[3] != 3:
        raise ValueError('vecs must be (replicates, frames, vectors, 3), got %s' % (sh,))
    R, F, V = sh[0], sh[1], sh[2]
    flat = np.ascontiguousarray(vecs, dtype=np.float32).reshape(R * F, V, 3)
    with _ctx(ctx).vectors(V, R * F) as rv:
        rv.append(flat)
        return _modes_result(rv, R, F, frame, None, mode)


def calculate_Ct_modes_from_files(vec_list, dt, tau, frame=None, ctx=None, mode=0):
    """calculate_Ct_modes on the chunks reformat_vecs_by_tau would form from the files (concat_with_chunk_starts: the tail of every
    file that does not fill a chunk of int(tau / dt) frames is skipped, exactly as for C(t))."""
    F = int(tau / dt)
    cat, starts, R = concat_with_chunk_starts(vec_list, F)
    if R < 1:
        raise ValueError('no trajectory holds a full block of memory time tau')
    with _ctx(ctx).vectors(cat.shape[1], cat.shape[0]) as rv:
        rv.append(cat)
        return _modes_result(rv, R, F, frame, starts, mode)


def calculate_Ct_modes_resident(rv, R, F, frame=None, mode=0, chunk_start=None):
    """calculate_Ct_modes of resident vectors (regular chunks r * F unless chunk_start is given); smean runs over the frames of the
    chunks used."""
    return _modes_result(rv, R, F, frame, chunk_start, mode)


def upload_shard(vec_list, frames_per_chunk=None, ctx=None):
    """The product path's single upload: this rank's vector range (srdist.my_range; everything in a single process) of the
    files' vectors, each file cut to whole chunks of frames_per_chunk frames when given (reformat_vecs_by_tau,
    calculate-Ct-from-traj.py:245-275), appended one after the other to a hip.ResidentVectors object.  Only the rank's
    columns cross PCIe, once; C(t) and the vector distribution then read the same planes.
    Returns (resident vectors, total vectors V, first vector i0, frames held)."""
    c = _ctx(ctx)
    V = vec_list[0].shape[1]
    i0, nloc = srdist.my_range(V) if srdist.world() > 1 else (0, V)
    used = []
    for v in vec_list:
        n = v.shape[0] if frames_per_chunk is None else (v.shape[0] // frames_per_chunk) * frames_per_chunk
        if n > 0:
            used.append((v, n))
    if not used:
        print("= = = ERROR: no trajectory holds a full block of memory time tau!", file=sys.stderr)
        sys.exit(1)
    N = sum(n for _, n in used)
    if nloc == 0:
        return None, V, i0, N
    rv = c.vectors(nloc, N)
    for v, n in used:
        rv.append(v[:n], v0=i0)
    return rv, V, i0, N


def chunk_table(vec_list, F):
    """(file index, first frame) of every whole chunk of F frames, in the order reformat_vecs_by_tau concatenates them."""
    return [(i, c * F) for i, v in enumerate(vec_list) for c in range(v.shape[0] // F)]


def calculate_Ct_chunk_sharded(vec_list, F, mode=0, ctx=None, sums_fn=None, finalize_fn=None):
    """C(t) with the replicate CHUNKS sharded over the ranks (fewer vectors than GPUs): this rank uploads the frames of its
    chunk range -- all vectors --, computes their raw sums, the (V, R, L) sums of all ranks are gathered and every rank
    runs the single-process mean / std kernel on them: the same bits as one process.
    sums_fn(list of (F, V, 3) chunks) -> (V, n, L) and finalize_fn((V, R, L)) -> (Ct, dCt) replace the GPU calls in the
    CPU test of the sharding logic (tests/test_cabi_and_dist.py)."""
    table = chunk_table(vec_list, F)
    R = len(table)
    if R < 1:
        print("= = = ERROR: no trajectory holds a full block of memory time tau!", file=sys.stderr)
        sys.exit(1)
    V = vec_list[0].shape[1]
    L = F // 2
    r0, nR = srdist.my_chunk_range(R)
    mine = [vec_list[i][f0:f0 + F] for i, f0 in table[r0:r0 + nR]]
    if nR == 0:
        sums = np.empty((V, 0, L))
    elif sums_fn is not None:
        sums = sums_fn(mine)
    else:
        with _ctx(ctx).vectors(V, nR * F) as rv:
            for c in mine:
                rv.append(c)
            sums = rv.ct_sums(nR, F, mode=mode)
    sums = srdist.gather_chunk_axis(sums, R)
    if finalize_fn is not None:
        return finalize_fn(sums)
    return _ctx(ctx).ct_finalize_sums(sums, F)


def calculate_Ct_resident(rv, V, R, F, mode=0):
    """calculate_Ct_Palmer of resident vectors (regular chunks r*F: the unused tails were dropped at upload); all ranks
    receive the whole (lags, V) arrays."""
    L = F // 2
    if rv is not None:
        Ct, dCt = rv.ct(R, F, mode=mode)
    else:
        Ct, dCt = np.empty((L, 0)), np.empty((L, 0))
    if srdist.world() > 1:
        return srdist.gather_rows(Ct, V, axis=1), srdist.gather_rows(dCt, V, axis=1)
    return Ct, dCt


def vector_distribution_resident(rv, V, N, q_rot=None, histBinX=72, delta_t=-1, tau_memory=-1):
    """vector_distribution() on resident vectors: same result dictionary."""
    edges = lambert_edges(histBinX)
    Fb = 0 if (delta_t < 0 or tau_memory < 0) else int(tau_memory / delta_t)
    if rv is not None:
        hist, vecsum, outer = rv.hist(q_rot, edges[0], edges[1], block_len=Fb, N_hist=N)
    else:
        nB = N // Fb if Fb else 1
        hist, vecsum, outer = np.empty((0, histBinX, int(histBinX / 2))), np.empty((0, 3)), np.empty((nB, 0, 6))
    if srdist.world() > 1:
        hist, vecsum = srdist.gather_rows(hist, V, axis=0), srdist.gather_rows(vecsum, V, axis=0)
        outer = srdist.gather_rows(outer, V, axis=1)
    mean = vecsum / N
    avgvec = mean / np.sqrt((mean ** 2).sum(-1))[..., np.newaxis]
    return dict(hist=hist, edges=edges, avgvec=avgvec, S2=S2_from_outer_sums(outer, Fb if Fb else N, blocked=bool(Fb)))


def lambert_edges(histBinX=72):
    """The bin edges numpy.histogramdd builds at calculate-Ct-from-traj.py:618 for
    bins=(histBinX, int(histBinX/2)), range=((-pi,pi),(-1,1))."""
    histBinY = int(histBinX / 2)
    return [np.linspace(-np.pi, np.pi, histBinX + 1), np.linspace(-1.0, 1.0, histBinY + 1)]


def vector_distribution(vecs, q_rot=None, histBinX=72, delta_t=-1, tau_memory=-1, ctx=None, v0=0, nV=None):
    """One pass replacing calculate-Ct-from-traj.py:541-646 for the Histogram storage mode:
    rotation into the PAF (rotate_vector_simd), mean vector (:579-583), Lambert-cylindrical histogram
    (:585-626) and calculate_S2_by_outerProduct (:96-145).

    vecs (N, V, 3) float32 (the 3-D array after the 4-D -> 3-D reshape at :535-536).
    Returns dict(hist (V,X,Y) float64, edges [X+1, Y+1], avgvec (V,3), S2 (V,2) or (V,))."""
    vecs = np.ascontiguousarray(vecs, dtype=np.float32)
    N = vecs.shape[0]
    edges = lambert_edges(histBinX)
    if delta_t < 0 or tau_memory < 0:
        Fb = 0
    else:
        Fb = int(tau_memory / delta_t)
    if srdist.world() > 1 and nV is None and v0 == 0:
        V = vecs.shape[1]
        i0, nloc = srdist.my_range(V)
        if nloc > 0:
            hist, vecsum, outer = _ctx(ctx).rotate_hist(vecs, q_rot, edges[0], edges[1], v0=i0, nV=nloc, block_len=Fb)
        else:
            nB = N // Fb if Fb else 1
            hist, vecsum, outer = np.empty((0, histBinX, int(histBinX / 2))), np.empty((0, 3)), np.empty((nB, 0, 6))
        hist, vecsum = srdist.gather_rows(hist, V, axis=0), srdist.gather_rows(vecsum, V, axis=0)
        outer = srdist.gather_rows(outer, V, axis=1)
    else:
        hist, vecsum, outer = _ctx(ctx).rotate_hist(vecs, q_rot, edges[0], edges[1], v0=v0, nV=nV, block_len=Fb)
    mean = vecsum / N
    avgvec = mean / np.sqrt((mean ** 2).sum(-1))[..., np.newaxis]
    return dict(hist=hist, edges=edges, avgvec=avgvec, S2=S2_from_outer_sums(outer, Fb if Fb else N, blocked=bool(Fb)))


def S2_from_outer_sums(outer, frames_per_block, blocked=True):
    """calculate_S2_by_outerProduct (calculate-Ct-from-traj.py:125-142) from per-block sums of
    xx,yy,zz,xy,xz,yz: S2 = 1.5*sum_ij <u_i u_j>^2 - 0.5; with blocks: mean and std/(sqrt(nBlocks)-1)."""
    m = outer / frames_per_block
    s = 1.5 * (m[..., 0] ** 2 + m[..., 1] ** 2 + m[..., 2] ** 2
               + 2.0 * (m[..., 3] ** 2 + m[..., 4] ** 2 + m[..., 5] ** 2)) - 0.5
    if not blocked:
        return s[0]
    nBlocks = s.shape[0]
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.stack((np.mean(s, axis=0), np.std(s, axis=0) / (np.sqrt(nBlocks) - 1.0)), axis=-1)


def vecnorm_NDarray(v, axis=-1):
    """transforms3d_supplement.py:40-52: normalise along an axis, 0/0 -> 0."""
    v = np.asarray(v)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.nan_to_num(v / np.linalg.norm(v, axis=axis, keepdims=True))


def rotate_vector_simd(v, q, ctx=None):
    """transforms3d_supplement.py:270-296 for v (N, V, 3) float32 and either one quaternion q (4,) or one per
    frame, q (N, 4) / (N, 1, 4) (numpy broadcasting over the vector axis): float64 result, rotation on the GPU."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    shp = v.shape
    q = np.asarray(q, dtype=np.float64)
    if q.ndim == 3 and q.shape[1] == 1:
        q = q[:, 0, :]
    if q.ndim == 2:
        q = vecnorm_NDarray(q)
    out = _ctx(ctx).rotate_vectors(v.reshape(-1, 1, 3) if v.ndim == 2 else v, q)
    return out.reshape(shp)


def detumble_vectors(vecs_lab, q_orient, ctx=None):
    """Body-frame vectors from lab-frame vectors and the orientation trajectory q_orient(t) (PLUMED colvar-qorient,
    float32 fields, plumedcolvario.py:24-81): v_body(t) = R(q(t))^-1 v_lab(t), i.e. rotate_vector_simd with the
    conjugate quaternion per frame.  Returns float32 like the vectors the superposition route produces
    (calculate-Ct-from-traj.py:64-86, 466-467)."""
    q = np.array(q_orient, dtype=np.float64)
    if q.ndim != 2 or q.shape[1] != 4 or q.shape[0] != np.shape(vecs_lab)[0]:
        raise ValueError('detumble_vectors: need one quaternion (w x y z) per frame, got %s for %d frames'
                         % (q.shape, np.shape(vecs_lab)[0]))
    q[:, 1:] *= -1.0
    return rotate_vector_simd(vecs_lab, q, ctx=ctx).astype(np.float32)


def obtain_XHvecs(xyz, indexX, indexH, ctx=None, bSuppressPrint=False):
    """obtain_XHvecs (calculate-Ct-from-traj.py:64-86) on a coordinate array instead of an MDTraj trajectory: xyz is
    traj.xyz (frames, atoms, 3) float32, indexX / indexH what topology.select() returned for the X and H selections.
    Unit vectors (x_H - x_X)/|x_H - x_X|, float32, 0/0 -> 0, computed on the GPU (bit-identical to the numpy expression)."""
    if not bSuppressPrint:
        print("= = = Obtaining XH-vectors from trajectory...")
    numX, numH = len(indexX), len(indexH)
    if numX == 0 or numH == 0:
        print("= = = ERROR: selection text failed to find atoms!")
        print("     ....debug: N(X) = %i , N(H) = %i" % (numX, numH))
        sys.exit(1)
    if numX != numH:
        print("= = = ERROR: selection text found different number of atoms!")
        print("     ....debug: N(X) = %i , N(H) = %i" % (numX, numH))
        sys.exit(1)
    lab, _, _ = _ctx(ctx).xh_vectors(xyz, indexX, indexH)
    return lab


def superpose_XHvecs(xyz, ref_xyz, fit_indices, indexX, indexH, ctx=None, want_quat=False):
    """The reference's two obtain_XHvecs calls around trj.center_coordinates(); trj.superpose(ref, frame=0,
    atom_indices=fit_indices) (calculate-Ct-from-traj.py:462-470) in one pass over the coordinates on the GPU:
    returns (vecXH lab frame, vecXHfit after the per-frame least-squares superposition [, rotation quaternions])."""
    lab, fitv, quat = _ctx(ctx).xh_vectors(xyz, indexX, indexH, fit_indices=fit_indices, ref_xyz=ref_xyz, want_quat=want_quat)
    return (lab, fitv, quat) if want_quat else (lab, fitv)
