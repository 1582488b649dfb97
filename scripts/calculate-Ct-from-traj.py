#!/usr/bin/env python3
"""
Drop-in for the reference's calculate-Ct-from-traj.py (run-all.bash:476-481): same flags, same output
files (<o>_Ctext.dat, <o>_Ctint.dat, <o>_vecHistogram.npz | _vecPhiTheta.npz|.dat, <o>_avgvec.dat,
<o>_S2.dat; with the [extension] --iRED also <o>_iRED_S2.dat, <o>_iRED_eig.dat and, with --binary, <o>_iRED_matrix.npz; with --iRED_Ct
also <o>_iRED_Ctint.dat, <o>_iRED_modeCt.dat and <o>_iRED_tau.dat; with the [extension] --crossCt --pairs FILE also <o>_crossCtint.dat
and <o>_crossPairs.dat; with the [extension] --dipolarCt also <o>_dipolarCtint.dat and <o>_dipolarDist.dat; with the
[extension] --dipolarCrossCt --pairs FILE also <o>_dipolarCrossCtint.dat and <o>_dipolarCrossPairs.dat; with the [extension] --noeMap
also <o>_noeMap.dat and, with --binary, <o>_noeMap.npz, with --noeLags / --noeLagMax on top of it <o>_noeMapCt.dat, and with --noesy on top of it <o>_noesy.dat and, with --binary,
<o>_noesy.npz; --noesyD in the place of --noesyTauC: the same files under anisotropic tumbling, --vecRot as the tensor's frame; with the [extension] --modeCt also <o>_modeCt.npz, with
--modeD on top of it <o>_modeAmp.dat and with --modeField on top of that <o>_modeRelax.dat).  C(t), the rotation into
the PAF, the spherical histogram, the mean vector and S2 are computed on the MI355X (libspinrelax_hip.so); this script only parses arguments and moves files.

Several GPUs: run under torchrun (`torchrun --nproc-per-node N scripts/calculate-Ct-from-traj.py ...`): rank r computes the
contiguous vector range spinrelax_amd.dist.shard_range gives it, the results are all-gathered (RCCL) and rank 0 writes the
same files a single process writes.

Trajectory input:
  * with MDTraj installed: -s <pdb> -f <xtc ...> exactly like the reference; MDTraj only reads the files and
    resolves the atom selections, the bond vectors, the centring and the per-frame superposition (reference lines
    64-86, 462-470) run on the GPU (csrc/sr_traj.hip);
  * without MDTraj (or for synthetic data): -f <file.npz|.npy>.  An .npz holds either raw coordinates --
    `xyz` (frames, atoms, 3) float32 like traj.xyz, `indexX`, `indexH` and, for the superposition, `ref_xyz` (atoms, 3)
    and `fit_indices` -- which go through the same GPU front end, or precomputed unit vectors `vecs` (frames, bonds, 3;
    body frame) with optional `vecs_lab` (lab frame for _Ctext.dat; defaults to `vecs`); plus `names` (resSeq per bond;
    default 2..V+1) and `dt` (ps; default --dt).  A .npy holds unit vectors.  -s is still parsed and ignored then.
    For --dipolarCt and --dipolarCrossCt the distances come from the same file: |x_H - x_X| of the coordinates; `dist` (frames, bonds) beside `vecs`, or
    the lengths of `vecs` without it; the lengths of the vectors of a .npy -- every other analysis of the same run still expects
    unit vectors.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spinrelax_amd import ct as hostct                      # noqa: E402
from spinrelax_amd import dist as srdist                    # noqa: E402
from spinrelax_amd import general_scripts as gs             # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description='Obtain the unit X-H vectors from one of more trajectories, and compute '
                                            'S^2, C(t) and the vector distribution on the GPU (Palmer memory-time chunks).',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('-s', type=str, dest='topfn', required=True, nargs='+', help='Topology PDB (reference frame for fits).')
    p.add_argument('-f', '--infn', type=str, dest='infn', required=True, nargs='+',
                   help='One or more trajectories, or .npy/.npz files of precomputed unit vectors.')
    p.add_argument('-o', '--outpref', type=str, dest='out_pref', default='out', help='Output file prefix.')
    p.add_argument('--split', type=int, dest='nSplitFrames', default=-1, help='Read trajectories in chunks of N frames (MDTraj input).')
    p.add_argument('-t', '--tau', type=float, dest='tau', default=None, help='Memory time (global tumbling estimate), same units as the trajectory.')
    p.add_argument('--prefact', type=float, dest='zeta', default=(1.02 / 1.04) ** 6, help='Zero-point vibration prefactor applied to S2 output.')
    p.add_argument('--S2', dest='bDoS2', action='store_true', default=False, help='Calculate order parameters S2.')
    p.add_argument('--Ct', dest='bDoCt', action='store_true', default=False, help='Calculate autocorrelation C(t).')
    p.add_argument('--vecDist', dest='bDoVecDistrib', action='store_true', default=False, help='Print the vector distribution in spherical coordinates.')
    p.add_argument('--binary', action='store_true', default=False, help='Numpy binary storage for the vector distribution.')
    p.add_argument('--vecHist', dest='bDoVecHist', action='store_true', default=False, help='Print the 2D histogram instead of all vectors.')
    p.add_argument('--histBin', type=int, default=72, help='Number of bins along phi; theta uses half this number.')
    p.add_argument('--vecAvg', dest='bDoVecAverage', action='store_true', default=False, help='Print the average unit XH-vector.')
    p.add_argument('--vecRot', dest='vecRotQ', type=str, default='', help='Rotation quaternion "w x y z" into the PAF frame.')
    p.add_argument('--Hsel', '--selection', type=str, dest='Hseltxt', default='name H', help='MDTraj selection of the H atoms.')
    p.add_argument('--Xsel', type=str, dest='Xseltxt', default='name N and not resname PRO', help='MDTraj selection of the X atoms.')
    p.add_argument('--fitsel', type=str, dest='fittxt', default='custom occupancy', help='MDTraj selection used for the superposition.')
    p.add_argument('--help_sel', action='store_true', help='Display help for selection texts and exit.')
    p.add_argument('--dt', type=float, default=10.0, help='[extension] frame spacing in ps for .npy vector input.')
    p.add_argument('--qfile', type=str, nargs='+', default=None,
                   help='[extension, SURVEY 8(f)-1] PLUMED colvar-qorient file(s), one per trajectory file (fields time q.w q.x q.y q.z): '
                        'the fitted (body-frame) vectors are the lab-frame vectors rotated on the GPU by the inverse orientation '
                        'quaternion of every frame, instead of coming from a superposition.')
    p.add_argument('--exact', action='store_true', help='[extension] float64 validation mode of the C(t) kernel.')
    p.add_argument('--iRED', dest='bDoIRED', action='store_true', default=False,
                   help='[extension] iRED order parameters (Prompers & Brueschweiler 2002; Gu, Li & Brueschweiler 2014) from the P2 '
                        'cross-correlation matrix of all lab-frame vectors: <o>_iRED_S2.dat, <o>_iRED_eig.dat; with --binary also '
                        '<o>_iRED_matrix.npz.  Single process only.')
    p.add_argument('--iRED_window', type=float, dest='ired_window', default=None,
                   help='[extension] averaging window of --iRED in the units of the trajectory; windows tile every file from its first '
                        'frame. Default: 5 tau when --tau is given, otherwise every file as a whole.')
    p.add_argument('--iRED_Ct', dest='bDoIREDCt', action='store_true', default=False,
                   help='[extension, needs --iRED] correlation functions of the iRED modes: <o>_iRED_Ctint.dat (per vector, the format of '
                        '_Ctint.dat, lags 1 .. F_w/2), <o>_iRED_modeCt.dat (per mode rank, lag 0 included), <o>_iRED_tau.dat (rank, mean '
                        'eigenvalue, correlation time); with --binary the .npz also holds Cm_w and the eigenvectors.  Windows of at '
                        'most 5461 frames.')
    p.add_argument('--iRED_modes', type=int, dest='ired_modes', default=5, help='[extension] number of global (tumbling) modes of --iRED.')
    p.add_argument('--crossCt', dest='bDoCrossCt', action='store_true', default=False,
                   help='[extension, needs --pairs and --tau] time-lagged P2 cross-correlation functions <P2(u_i(t).u_j(t+k))> between pairs of '
                        'the fitted vectors, chunked by --tau like --Ct: <o>_crossCtint.dat (the format of _Ctint.dat, one block per pair, '
                        'labelled by the ordinal of the pair; calculate-fitted-Ct.py reads it) and <o>_crossPairs.dat (ordinal, i, j, their '
                        'residue ids, the equal-time value P0 = <P2(u_i.u_j)> and its standard error over the chunks).  Dot products do '
                        'not change under a rotation: --vecRot has no effect on these files.  Any --tau that --Ct accepts (up to '
                        '262144 frames per chunk: long chunks run by blocked transforms).  Single process only.')
    p.add_argument('--pairs', type=str, dest='pairs_fn', default=None,
                   help='[extension] pair file of --crossCt: two integers per line, 0-based indices into the list of vectors; # starts a comment.')
    p.add_argument('--asym', dest='bCrossAsym', action='store_true', default=False,
                   help='[extension] --crossCt writes C_ij and C_ji of every pair as two blocks, one after the other, instead of their mean.')
    p.add_argument('--dipolarCt', dest='bDoDipolarCt', action='store_true', default=False,
                   help='[extension, needs --tau] distance-weighted dipolar correlation functions of flexible spin pairs, '
                        '<P2(u(t).u(t+k)) r(t)^-3 r(t+k)^-3> / <r^-6>, chunked by --tau like --Ct: <o>_dipolarCtint.dat (the format of '
                        '_Ctint.dat, labelled by residue; calculate-fitted-Ct.py reads it) and <o>_dipolarDist.dat (resid, the effective '
                        'distances <r^-6>^(-1/6) and <r^-3>^(-1/3) in the units of the input, and the radial order parameter '
                        '<r^-3>^2 / <r^-6>).  Vector-file input only (.npy/.npz): distances from `xyz`, from `dist` or from the lengths '
                        'of the vectors; then the other analyses of the run still expect unit vectors.  Any --tau that --Ct accepts (up to 262144 frames per '
                        'chunk: chunks beyond 10016 frames run by blocked transforms).  '
                        '--exact: float64 throughout.  Dot products and distances do not change under a rotation: --vecRot has no '
                        'effect on these files.  Single process only.')
    p.add_argument('--dipolarCrossCt', dest='bDoDipolarCrossCt', action='store_true', default=False,
                   help='[extension, needs --pairs and --tau] distance-weighted P2 cross-correlation functions between pairs of flexible '
                        'spin pairs, <P2(u_i(t).u_j(t+k)) r_i(t)^-3 r_j(t+k)^-3> / sqrt(<r_i^-6><r_j^-6>), the function of dipole-dipole '
                        'cross-correlated relaxation: --crossCt with the distance weights of --dipolarCt.  <o>_dipolarCrossCtint.dat (the '
                        'format of _crossCtint.dat, one block per pair) and <o>_dipolarCrossPairs.dat (ordinal, i, j, their residue ids, '
                        'the equal-time value P0 and its standard error over the chunks, and the effective distances <r^-6>^(-1/6) of '
                        'the two vectors).  Pairs from --pairs, --asym as for --crossCt; distances as for --dipolarCt (vector-file input '
                        'only).  Any --tau that --Ct accepts (chunks beyond 4896 frames run by blocked transforms).  --exact: float64 throughout.  --vecRot has no effect on these files.  '
                        'Single process only.')
    p.add_argument('--noeMap', dest='bDoNoeMap', action='store_true', default=False,
                   help='[extension] all-pairs dipolar map (Brueschweiler et al. 1992; Peter, Daura & van Gunsteren 2001): for EVERY pair of '
                        'the atoms `indexP` of an .npz coordinate file (default: the union of `indexX` and `indexH`; optional `namesP`) the '
                        'effective distances <r^-6>^(-1/6) and <r^-3>^(-1/3), the order parameter S2 of the pair vector -- the plateau '
                        'of the --dipolarCt function -- and the radial order parameter, in the frame of the superposition onto `ref_xyz` '
                        'over `fit_indices` (without them: the lab frame, S2 then includes overall tumbling): <o>_noeMap.dat with the '
                        'columns i j name_i name_j reff6 dreff6 reff3 S2 dS2 S2rad; with --binary also <o>_noeMap.npz.  Errors over the '
                        '--tau chunks, one block per file without --tau.  --exact: float64 throughout.  The screening step in front '
                        'of --dipolarCt.  Single process only.')
    p.add_argument('--noeCutoff', type=float, dest='noe_cutoff', default=None,
                   help='[extension] --noeMap lists only the pairs with reff6 <= this distance, in the units of the coordinates.')
    p.add_argument('--noeLags', type=str, dest='noe_lags', default=None,
                   help='[extension] with --noeMap: the dipolar correlation function C_dd(k) of EVERY pair at these lags, in frames, e.g. '
                        '"1 2 4 8 16" (integers >= 0, strictly increasing, at most 64, the largest below the frames of a --tau block), and '
                        'from them the internal correlation time tau_e of every pair (the Lipari-Szabo integral of (C_dd - S2) / (1 - S2) by '
                        'the trapezoid rule): <o>_noeMapCt.dat with the columns i j name_i name_j tau_e dtau_e and one C_dd column per lag, '
                        'times in ps; with --binary lags, G, Cdd, dCdd, tau_e and dtau_e also go into <o>_noeMap.npz.')
    p.add_argument('--noeLagMax', type=int, dest='noe_lag_max', default=None,
                   help='[extension] with --noeMap, in the place of --noeLags: about --noeLagCount log-spaced lags from 1 to this many frames.')
    p.add_argument('--noeLagCount', type=int, dest='noe_lag_count', default=None,
                   help='[extension] --noeLagMax: the number of lags (default 12; neighbours that round to the same frame are merged).')
    p.add_argument('--noesy', dest='bDoNoesy', action='store_true', default=False,
                   help='[extension] with --noeMap: NOESY cross-peak intensities of the map\'s spins by the full relaxation matrix '
                        '(Macura & Ernst 1980; Keepers & James 1984; model-free rates from <r^-6> and S2, Brueschweiler et al. 1992), spin '
                        'diffusion included: A(tau_m) = exp(-R tau_m) at the mixing times of --noesyMix.  <o>_noesy.dat with the columns '
                        'i j name_i name_j sigma and one column per mixing time, the diagonal rows i = j included (--noeCutoff applies to '
                        'the pairs); with --binary also <o>_noesy.npz.  Needs --noesyMix, --noesyField and --noesyTauC (isotropic tumbling) or --noesyD (anisotropic), '
                        'protons only, single process only.')
    p.add_argument('--noesyMix', type=str, dest='noesy_mix', default=None, help='[extension] --noesy: the mixing times in seconds, e.g. "0.05 0.1 0.2".')
    p.add_argument('--noesyField', type=float, dest='noesy_field', default=None, help='[extension] --noesy: the proton frequency of the spectrometer in MHz.')
    p.add_argument('--noesyTauC', type=float, dest='noesy_tauc', default=None, help='[extension] --noesy: the overall correlation time tau_c in seconds.')
    p.add_argument('--noesyD', type=str, dest='noesy_D', default=None,
                   help='[extension] --noesy under anisotropic tumbling, in the place of --noesyTauC: the rotational diffusion tensor as '
                        '"Diso aniso [rhomb]", Diso in 1/s (the convention of calculate-relaxations-from-Ct.py).  The map then also holds the '
                        'mode sums of every pair in the frame of --vecRot, the quaternion into the tensor\'s principal-axis frame (identity '
                        'without it), lag 0 is put in front of the lags, and with --noesyTauEMap every mode of every pair has its own tau_e.  '
                        'With --binary H, H_blocks and frame also go into <o>_noeMap.npz.')
    p.add_argument('--noesyTauE', type=float, dest='noesy_taue', default=None,
                   help='[extension] --noesy: the correlation time of the internal motion tau_e in seconds (default 1e-10).')
    p.add_argument('--noesyTauEMap', dest='noesy_taue_map', action='store_true', default=False,
                   help='[extension] --noesy: every pair with its own tau_e, the one --noeLags / --noeLagMax give (ps, converted to '
                        'seconds; floored at 1e-12 s), in the place of one --noesyTauE for all pairs.')
    p.add_argument('--noesyLeak', type=float, dest='noesy_leak', default=None,
                   help='[extension] --noesy: a leakage rate in 1/s added to every diagonal element (default 0).')
    p.add_argument('--noesyUnit', type=str, dest='noesy_unit', default=None, choices=('nm', 'A'),
                   help='[extension] --noesy: the unit of the coordinates (default nm, MDTraj\'s).')
    p.add_argument('--noesyGroups', type=str, dest='noesy_groups', default=None,
                   help='[extension] --noesy: a file with one group of equivalent or unresolved spins per line (positions in the list of '
                        'selected atoms); the intensities summed over the groups go to <o>_noesyGroups.dat.')
    p.add_argument('--modeCt', dest='bDoModeCt', action='store_true', default=False,
                   help='[extension] C(t) of the fitted vectors split into the five tumbling modes of an anisotropic diffusion tensor: the six '
                        'mode sums of every vector at the lags 0 .. tau/2 in the frame of --vecRot, the quaternion into the tensor\'s '
                        'principal-axis frame (identity without it), to <o>_modeCt.npz (H, dH, smean, lags, dt, frame).  They do not depend '
                        'on the tensor.  Needs --tau, chunks of at most 7968 frames.  --exact: float64 throughout.')
    p.add_argument('--modeD', type=str, dest='mode_D', default=None,
                   help='[extension] --modeCt: the rotational diffusion tensor as "Diso aniso [rhomb]", Diso in 1/s, parsed like --noesyD; '
                        'also writes <o>_modeAmp.dat with the amplitudes a_m(0), the plateaus c_m and S2 = sum c_m of every vector.')
    p.add_argument('--modeField', type=float, dest='mode_field', default=None,
                   help='[extension] --modeCt --modeD: the proton frequency of the spectrometer in MHz; also writes <o>_modeRelax.dat with '
                        'R1, R2 and NOE of every vector (15N-1H, the constants of calculate-relaxations-from-Ct.py).')
    return p


TIME_UNIT_S = 1e-12       # the times of a run (dt of the input, --dt, --tau) are in ps


def mode_tensor(args):
    """--modeD "Diso aniso [rhomb]" -> (Dx, Dy, Dz) in 1/s, --noesyD's rule (noesy_tensor); None for anything else"""
    return noesy_tensor(argparse.Namespace(noesy_D=args.mode_D))


def check_mode_args(args):
    """the --mode* flags that do not fit together: an error message and exit, before any GPU work"""
    def fail(msg):
        print("= = = ERROR: %s" % msg, file=sys.stderr)
        sys.exit(1)
    if not args.bDoModeCt:
        for name, v in (('--modeD', args.mode_D), ('--modeField', args.mode_field)):
            if v is not None:
                fail("%s belongs to --modeCt; give both." % name)
        return
    if args.tau is None:
        fail("--modeCt needs --tau: the functions are block averages over the memory time.")
    if args.mode_field is not None and args.mode_D is None:
        fail("--modeField needs --modeD: the rates need the tumbling.")
    if args.mode_D is not None and mode_tensor(args) is None:
        fail("--modeD must be \"Diso aniso [rhomb]\" with Diso > 0 in 1/s and a tensor with Dx, Dy, Dz > 0; got '%s'." % args.mode_D)
    if args.mode_field is not None and not (np.isfinite(args.mode_field) and args.mode_field > 0):
        fail("--modeField must be > 0.")
    if args.vecRotQ != '':
        try:
            q = np.array([float(v) for v in args.vecRotQ.split()])
        except ValueError:
            q = np.zeros(0)
        if q.shape != (4,) or not np.all(np.isfinite(q)) or abs(float(q @ q) - 1.0) > 1e-6:
            fail("--modeCt takes --vecRot as the unit quaternion \"w x y z\" into the tensor's frame; got '%s'." % args.vecRotQ)


def run_mode_ct(args, out_pref, rv_fit, resXH, R, F, deltaT, q_rot):
    """--modeCt: the mode-resolved C(t) of the fitted vectors and, with --modeD / --modeField, amplitudes and rates"""
    from spinrelax_amd import modes
    print("= = = Conducting mode-resolved C(t) analysis of the fitted vectors using Palmer's approach.")
    try:
        res = hostct.calculate_Ct_modes_resident(rv_fit, R, F, frame=q_rot, mode=1 if args.exact else 0)
    except (ValueError, hostct.hip.SpinRelaxHipError) as exc:      # a zero-length vector, a chunk beyond the staged kernel
        print("= = = ERROR: %s" % exc, file=sys.stderr)
        sys.exit(1)
    np.savez(out_pref + '_modeCt.npz', H=res['H'], dH=res['dH'], smean=res['smean'], lags=res['lags'], dt=float(deltaT), frame=res['frame'],
             names=np.array(resXH))
    if args.mode_D is not None:
        D = mode_tensor(args) * TIME_UNIT_S                         # 1/s -> 1/ps, the unit of dt
        a, c, _ = modes.amplitudes(res, D)
        with open(out_pref + '_modeAmp.dat', 'w') as fp:
            print("# resid a_0(0) .. a_4(0) c_0 .. c_4 S2", file=fp)
            for n in range(a.shape[1]):
                print("%s %s %s %.8g" % (resXH[n], ' '.join('%.8g' % x for x in a[0, n]), ' '.join('%.8g' % x for x in c[n]), c[n].sum()), file=fp)
        if args.mode_field is not None:
            rel = modes.relaxation(res, D, float(deltaT), args.mode_field)
            with open(out_pref + '_modeRelax.dat', 'w') as fp:
                print("# resid R1 R2 NOE", file=fp)
                for n in range(a.shape[1]):
                    print("%s %.8g %.8g %.8g" % (resXH[n], rel['R1'][n], rel['R2'][n], rel['NOE'][n]), file=fp)
    print("      ...complete.")


def check_noe_lag_args(args):
    """the --noeLag* flags that do not fit together or give no lag list: an error message and exit, before any GPU work; returns the
    lags in frames (int64), None without them"""
    def fail(msg):
        print("= = = ERROR: %s" % msg, file=sys.stderr)
        sys.exit(1)
    given = [n for n, v in (('--noeLags', args.noe_lags), ('--noeLagMax', args.noe_lag_max), ('--noeLagCount', args.noe_lag_count))
             if v is not None]
    if not given:
        return None
    if not args.bDoNoeMap:
        fail("%s belongs to --noeMap; give both." % given[0])
    if args.noe_lags is not None and args.noe_lag_max is not None:
        fail("--noeLags and --noeLagMax both give the lags; give one of them.")
    if args.noe_lag_count is not None and args.noe_lag_max is None:
        fail("--noeLagCount belongs to --noeLagMax; give both.")
    if args.noe_lag_max is not None:
        n = 12 if args.noe_lag_count is None else args.noe_lag_count
        if args.noe_lag_max < 1 or n < 2 or n > 64:
            fail("--noeLagMax must be >= 1 and --noeLagCount 2 .. 64; got %d and %d." % (args.noe_lag_max, n))
        from spinrelax_amd.noe import log_lags
        return log_lags(args.noe_lag_max, n)
    try:
        lags = np.array([int(w) for w in args.noe_lags.split()], dtype=np.int64)
    except ValueError:
        lags = np.zeros(0, dtype=np.int64)
    if lags.size < 1 or lags.size > 64 or lags[0] < 0 or np.any(np.diff(lags) <= 0) or lags[-1] >= 2 ** 31:
        fail("--noeLags must list 1 .. 64 lags in frames, integers >= 0 and strictly increasing; got '%s'." % args.noe_lags)
    return lags


def noesy_tensor(args):
    """--noesyD "Diso aniso [rhomb]" -> (Dx, Dy, Dz) in 1/s through _hostmath.ellipsoid_from_iso; None for anything else"""
    from spinrelax_amd._hostmath import ellipsoid_from_iso
    try:
        w = [float(v) for v in args.noesy_D.split()]
    except ValueError:
        return None
    if len(w) not in (2, 3) or not np.all(np.isfinite(w)) or not w[0] > 0 or not w[1] > 0:
        return None
    D = np.array(ellipsoid_from_iso(w[0], w[1], w[2] if len(w) == 3 else 0.0), dtype=np.float64)
    return D if np.all(np.isfinite(D)) and np.all(D > 0) else None


def check_noesy_args(args):
    """the --noesy* flags that do not fit together: an error message and exit, before any GPU work; returns the mixing times"""
    given = [n for n, v in (('--noesyMix', args.noesy_mix), ('--noesyField', args.noesy_field), ('--noesyTauC', args.noesy_tauc),
                            ('--noesyD', args.noesy_D), ('--noesyTauE', args.noesy_taue), ('--noesyLeak', args.noesy_leak), ('--noesyUnit', args.noesy_unit),
                            ('--noesyGroups', args.noesy_groups), ('--noesyTauEMap', args.noesy_taue_map or None)) if v is not None]
    if not args.bDoNoesy:
        if given:
            print("= = = ERROR: %s belongs to --noesy; give both." % given[0], file=sys.stderr)
            sys.exit(1)
        return None
    if not args.bDoNoeMap:
        print("= = = ERROR: --noesy works on the map of --noeMap; give both.", file=sys.stderr)
        sys.exit(1)
    if args.noesy_D is not None and args.noesy_tauc is not None:
        print("= = = ERROR: --noesyD and --noesyTauC both describe the tumbling; give one of them.", file=sys.stderr)
        sys.exit(1)
    for name, v in (('--noesyMix', args.noesy_mix), ('--noesyField', args.noesy_field),
                    ('--noesyTauC' if args.noesy_D is None else '--noesyD', args.noesy_tauc if args.noesy_D is None else args.noesy_D)):
        if v is None:
            print("= = = ERROR: --noesy needs %s." % name, file=sys.stderr)
            sys.exit(1)
    if args.noesy_D is not None and noesy_tensor(args) is None:
        print("= = = ERROR: --noesyD must be \"Diso aniso [rhomb]\" with Diso > 0 in 1/s and a tensor with Dx, Dy, Dz > 0; got '%s'."
              % args.noesy_D, file=sys.stderr)
        sys.exit(1)
    if args.noesy_D is not None and args.vecRotQ != '':
        try:
            q = np.array([float(v) for v in args.vecRotQ.split()])
        except ValueError:
            q = np.zeros(0)
        if q.shape != (4,) or not np.all(np.isfinite(q)) or abs(np.dot(q, q) - 1.0) > 1e-6:
            print("= = = ERROR: --noesyD takes --vecRot as the unit quaternion \"w x y z\" into the tensor's frame; got '%s'." % args.vecRotQ,
                  file=sys.stderr)
            sys.exit(1)
    try:
        mix = np.array([float(w) for w in args.noesy_mix.split()])
    except ValueError:
        mix = np.zeros(0)
    if mix.size < 1 or not np.all(np.isfinite(mix)) or np.any(mix < 0):
        print("= = = ERROR: --noesyMix must list mixing times in seconds, finite and >= 0; got '%s'." % args.noesy_mix, file=sys.stderr)
        sys.exit(1)
    if not args.noesy_field > 0 or (args.noesy_tauc is not None and not args.noesy_tauc > 0) or (args.noesy_taue is not None and not args.noesy_taue > 0) \
            or (args.noesy_leak is not None and not args.noesy_leak >= 0):
        print("= = = ERROR: --noesyField, --noesyTauC and --noesyTauE must be > 0 and --noesyLeak >= 0.", file=sys.stderr)
        sys.exit(1)
    if args.noesy_groups is not None and not os.path.isfile(args.noesy_groups):
        print("= = = ERROR: --noesyGroups file %s does not exist." % args.noesy_groups, file=sys.stderr)
        sys.exit(1)
    if args.noesy_taue_map:
        if args.noesy_taue is not None:
            print("= = = ERROR: --noesyTauEMap and --noesyTauE both give tau_e; give one of them.", file=sys.stderr)
            sys.exit(1)
        if args.noe_lags is None and args.noe_lag_max is None:
            print("= = = ERROR: --noesyTauEMap takes tau_e from the lagged map; give --noeLags or --noeLagMax.", file=sys.stderr)
            sys.exit(1)
    return mix


def run_noesy(args, out_pref, res, names):
    """--noesy: the intensities of the map `res` at the mixing times of --noesyMix through spinrelax_amd.noesy"""
    from spinrelax_amd import noesy
    mix = check_noesy_args(args)
    print("= = = Conducting the relaxation-matrix NOESY calculation of %i spins at %i mixing times." % (res['index'].size, mix.size))
    tau_e = 1e-10 if args.noesy_taue is None else args.noesy_taue
    D = None if args.noesy_D is None else noesy_tensor(args)
    if args.noesy_taue_map:
        # the map's tau_e and dt are in the time unit of the run
        res = dict(res, tau_e=res['tau_e'] * TIME_UNIT_S, dt=res['dt'] * TIME_UNIT_S)
        tau_e = 'map' if D is None else 'modes'
    try:
        out = noesy.noesy(res, mix, args.noesy_field, args.noesy_tauc, tau_e=tau_e, D=D,
                          leak=0.0 if args.noesy_leak is None else args.noesy_leak, unit=args.noesy_unit or 'nm')
        rows = noesy.write_noesy(out_pref + '_noesy.dat', out, names=names, reff6=res['reff6'], cutoff=args.noe_cutoff)
        if args.noesy_groups is not None:
            groups = noesy.read_groups(args.noesy_groups)
            grp = dict(index=np.arange(len(groups)), R=noesy.sum_groups(out['R'], groups), A=noesy.sum_groups(out['A'], groups),
                       mixing_times=out['mixing_times'])
            noesy.write_noesy(out_pref + '_noesyGroups.dat', grp, names=['G%d' % g for g in range(len(groups))])
    except (ValueError, hostct.hip.SpinRelaxHipError) as exc:
        print("= = = ERROR: %s" % exc, file=sys.stderr)
        sys.exit(1)
    if args.binary:
        np.savez(out_pref + '_noesy.npz', **{k: out[k] for k in ('R', 'sigma', 'rho', 'A', 'mixing_times', 'index', 'pairs')})
    print("      ...%i rows written; complete." % rows)


def run_noe_map(args, out_pref):
    """--noeMap: the coordinates of all files, one after the other, through spinrelax_amd.noe; the blocks are the --tau chunks of
    every file (a tail that does not fill one is dropped), without --tau every file as a whole; with --noeLags / --noeLagMax also the
    correlation functions and tau_e of every pair"""
    from spinrelax_amd import ired, noe
    lags = check_noe_lag_args(args)
    modes = dict()
    if args.bDoNoesy and args.noesy_D is not None:
        # anisotropic tumbling: the mode sums in the frame of --vecRot, from lag 0 on
        modes = dict(modes=True, frame=np.array([float(v) for v in args.vecRotQ.split()]) if args.vecRotQ != '' else None)
        if lags is not None and lags[0] != 0:
            lags = np.concatenate([[0], lags])
    xyz, frames, first = [], [], None
    for fn in args.infn:
        z = np.load(fn, allow_pickle=True) if fn.endswith('.npz') else {}
        if 'xyz' not in z:
            print("= = = ERROR: --noeMap needs .npz coordinate input that holds `xyz`; %s does not." % fn, file=sys.stderr)
            sys.exit(1)
        if first is None:
            first = z
        xyz.append(np.ascontiguousarray(z['xyz'], dtype=np.float32))
        frames.append(xyz[-1].shape[0])
    z = first
    if 'indexP' in z:
        index = np.asarray(z['indexP'], dtype=np.int64)
    elif 'indexX' in z and 'indexH' in z:
        index = np.union1d(np.asarray(z['indexX'], dtype=np.int64), np.asarray(z['indexH'], dtype=np.int64))
    else:
        print("= = = ERROR: --noeMap needs `indexP`, or `indexX` and `indexH`, in the coordinate file.", file=sys.stderr)
        sys.exit(1)
    names = [str(n) for n in z['namesP']] if 'namesP' in z else None
    dt = float(z['dt']) if 'dt' in z else float(args.dt)
    if args.tau is not None and dt > 0.5 * args.tau:
        print("= = = ERROR: delta-t form the trajectory is too small relative to tau! %g vs. %g" % (dt, args.tau), file=sys.stderr)
        sys.exit(1)
    blocks = ired.ired_windows(frames, dt, window=args.tau)
    if blocks[0].size < 1:
        print("= = = ERROR: no trajectory holds a full block of memory time tau!", file=sys.stderr)
        sys.exit(1)
    allxyz = xyz[0] if len(xyz) == 1 else np.concatenate(xyz, axis=0)
    mode = 1 if args.exact else 0
    print("= = = Conducting the all-pairs dipolar map of %i atoms (%i pairs) over %i blocks." % (index.size, noe.n_pairs(index.size), blocks[0].size))
    try:
        if 'ref_xyz' in z and 'fit_indices' in z:
            res = noe.dipolar_map_superposed(allxyz, z['ref_xyz'], z['fit_indices'], index, blocks=blocks, mode=mode, lags=lags, dt=dt, **modes)
        else:
            print("= = = WARNING: no `ref_xyz` / `fit_indices` in the input: the map is computed in the lab frame and its S2 includes "
                  "overall tumbling.", file=sys.stderr)
            res = noe.dipolar_map(allxyz, index, blocks=blocks, mode=mode, lags=lags, dt=dt, **modes)
        rows = noe.write_map(out_pref + '_noeMap.dat', res, names=names, cutoff=args.noe_cutoff)
        if lags is not None:
            noe.write_map_ct(out_pref + '_noeMapCt.dat', res, names=names, cutoff=args.noe_cutoff)
    except (ValueError, hostct.hip.SpinRelaxHipError) as exc:        # coinciding atoms, a bad index list, a map beyond the device
        print("= = = ERROR: %s" % exc, file=sys.stderr)
        sys.exit(1)
    if args.binary:
        keep = ('pairs', 'index', 'A6', 'A3', 'T', 'reff6', 'reff3', 'S2', 'S2rad', 'dS2', 'dreff6', 'dreff3', 'A6_b', 'A3_b', 'T_b',
                'reff6_b', 'reff3_b', 'S2_b', 'S2rad_b', 'block_len', 'sums')
        if lags is not None:
            keep += ('lags', 'G', 'Cdd', 'dCdd', 'tau_e', 'dtau_e')
        if modes:
            keep += ('H', 'H_blocks', 'frame')
        np.savez(out_pref + '_noeMap.npz', block_start=blocks[0], **{k: res[k] for k in keep})
    print("      ...%i of %i pairs written; complete." % (rows, res['reff6'].size))
    if args.bDoNoesy:
        run_noesy(args, out_pref, res, names)
    return all(('indexX' in np.load(fn, allow_pickle=True)) for fn in args.infn)


def load_distance_files(files, frames_per_chunk):
    """The distances of --dipolarCt from .npy / .npz vector input, cut to whole chunks like the vectors (hostct.upload_shard) and
    concatenated: (frames kept, bonds) float32, or None when the lengths of the vectors are the distances."""
    out = []
    for fn in files:
        d = None
        if not fn.endswith('.npy'):
            z = np.load(fn, allow_pickle=True)
            if 'xyz' in z:
                x = np.asarray(z['xyz'], dtype=np.float64)
                d = np.linalg.norm(x[:, np.asarray(z['indexH'])] - x[:, np.asarray(z['indexX'])], axis=-1)
            elif 'dist' in z:
                d = np.asarray(z['dist'])
                if d.ndim != 2 or d.shape != z['vecs'].shape[:2]:
                    raise ValueError('%s: dist must be (frames, bonds) = %s, got %s' % (fn, z['vecs'].shape[:2], d.shape))
        out.append(d)
    if all(d is None for d in out):
        return None
    if any(d is None for d in out):
        raise ValueError('some of the files hold distances and some do not')
    return np.ascontiguousarray(np.concatenate([d[:(d.shape[0] // frames_per_chunk) * frames_per_chunk] for d in out], axis=0), dtype=np.float32)


def load_vector_files(files, default_dt):
    """.npy / .npz vector input -> (resXH, [vecXH per file], [vecXHfit per file], deltaT)."""
    resXH, lab, body, dt = None, [], [], None
    for fn in files:
        if fn.endswith('.npy'):
            v = np.load(fn)
            names, vl, d = None, v, default_dt
        else:
            z = np.load(fn, allow_pickle=True)
            if 'xyz' in z:
                # raw coordinates (traj.xyz) + the index lists MDTraj's selections would give: the front end
                # (obtain_XHvecs, centre + superpose, calculate-Ct-from-traj.py:64-86, 462-470) runs on the GPU
                print("= = = Reading coordinate file %s ..." % fn)
                if 'ref_xyz' in z:
                    vl, v = hostct.superpose_XHvecs(z['xyz'], z['ref_xyz'], z['fit_indices'], z['indexX'], z['indexH'])
                    print("= = = Molecule centered and fitted.")
                else:
                    v = vl = hostct.obtain_XHvecs(z['xyz'], z['indexX'], z['indexH'])
            else:
                v = z['vecs']
                vl = z['vecs_lab'] if 'vecs_lab' in z else v
            names = list(z['names']) if 'names' in z else None
            d = np.float32(z['dt']) if 'dt' in z else np.float32(default_dt)      # float32 like MDTraj's frame times (see load_mdtraj)
        if v.ndim != 3 or v.shape[2] != 3:
            print("= = = ERROR: vector file %s does not hold a (frames, bonds, 3) array!" % fn, file=sys.stderr)
            sys.exit(1)
        names = list(range(2, v.shape[1] + 2)) if names is None else [int(x) for x in names]
        if resXH is None:
            resXH, dt = names, d
        elif dt != d or resXH != names:
            print("= = = ERROR: Differences in trajectories have been detected! Aborting.", file=sys.stderr)
            sys.exit(1)
        body.append(np.ascontiguousarray(v, dtype=np.float32))
        lab.append(np.ascontiguousarray(vl, dtype=np.float32))
    return resXH, lab, body, dt


def load_mdtraj(args, frames_per_chunk_of):
    """The reference's loader (calculate-Ct-from-traj.py:396-498) on top of MDTraj, STREAMING: MDTraj reads the file (in
    chunks of --split frames, `md.iterload`, like the reference's :426-453, or 1000 frames otherwise) and resolves the
    selections; every chunk's coordinates go to the GPU, where the bond vectors, the centring and the per-frame superposition
    are computed and APPENDED to this rank's resident vectors (spinrelax_amd.hip.ResidentVectors) -- the host never holds
    more than one chunk of coordinates and no vectors at all.  A file's tail that does not fill a block of memory time is
    cut when the file ends (reformat_vecs_by_tau, :259-272).  frames_per_chunk_of(dt) -> frames per block or None.
    Returns (resXH, lab vectors, fitted vectors, deltaT, total vectors V, first vector i0, frames kept, frames kept of each file)."""
    try:
        import mdtraj as md
    except ImportError:
        print("= = = ERROR: MDTraj is not installed; give precomputed vectors as .npy/.npz to -f instead.", file=sys.stderr)
        sys.exit(1)
    from spinrelax_amd import hip

    def select(traj):
        iX = traj.topology.select(args.Xseltxt)
        iH = traj.topology.select(args.Hseltxt)
        if len(iX) == 0 or len(iH) == 0 or len(iX) != len(iH):
            print("= = = ERROR: selection text failed to find matching atoms! N(%s) = %i , N(%s) = %i"
                  % (args.Xseltxt, len(iX), args.Hseltxt, len(iH)), file=sys.stderr)
            sys.exit(1)
        return iX, iH

    def fit_indices(ref, fn):
        if args.fittxt == 'custom occupancy':
            pdb = md.formats.pdb.pdbstructure.PdbStructure(open(fn))
            mask = [a.get_occupancy() for a in pdb.iter_atoms()]
            inds = ref.topology.select('all')
            return [inds[i] for i in range(len(mask)) if mask[i] > 0.0]
        return ref.topology.select(args.fittxt)

    ctx = hip.default_context()
    resXH, dt, lab, fit, V, i0, nloc = None, None, None, None, None, 0, 0
    kept = []
    for i, fn in enumerate(args.infn):
        top = args.topfn[i] if len(args.topfn) > 1 else args.topfn[0]
        ref = md.load(top)
        fi = fit_indices(ref, top)
        nchunk = args.nSplitFrames if args.nSplitFrames > 0 else 1000
        file_start = 0 if lab is None else lab.frames
        nfile = 0
        iX = iH = None
        for trj in md.iterload(fn, chunk=nchunk, top=top):
            if iX is None:
                # names, selections and the time step come from a file's FIRST chunk only, as in the reference (:436-438):
                # a later chunk may hold a single frame (MDTraj's .timestep raises for it) and float32 frame times of
                # later chunks give a time step that differs from the first one in its last bits
                names = [trj.topology.atom(k).residue.resSeq for k in trj.topology.select(args.Hseltxt)]
                d = trj.timestep          # MDTraj's np.float32, KEPT float32: the reference's int(tau/dt) and int(0.5*tau/dt)
                                          # (:241, :255) are float32 divisions under NumPy >= 2 -- tau = 10, dt = 0.1 gives 100, not 99
                iX, iH = select(trj)
                if resXH is None:
                    resXH, dt, V = names, d, len(iX)
                    i0, nloc = srdist.my_range(V) if srdist.world() > 1 else (0, V)
                    if nloc > 0:
                        lab, fit = ctx.vectors(nloc), ctx.vectors(nloc)
                elif dt != d or resXH != names:
                    print("= = = ERROR: Differences in trajectories have been detected! Aborting.", file=sys.stderr)
                    print("      ...delta-t: %g vs.%g " % (dt, d), file=sys.stderr)
                    print("      ...n-bonds: %g vs.%g " % (V, len(iX)), file=sys.stderr)
                    sys.exit(1)
            if nloc > 0:
                hip.append_xyz(ctx, lab, fit, trj.xyz, iX[i0:i0 + nloc], iH[i0:i0 + nloc], fi, ref.xyz[0])
            nfile += trj.xyz.shape[0]
        if iX is None:
            print("= = = ERROR: trajectory file %s holds no frames!" % fn, file=sys.stderr)
            sys.exit(1)
        F = frames_per_chunk_of(dt)
        keep = nfile if F is None else (nfile // F) * F
        if nloc > 0 and keep != nfile:
            lab.truncate(file_start + keep)
            fit.truncate(file_start + keep)
        kept.append(keep)
        print("= = = Molecule centered and fitted: %s, %i frames read, %i kept." % (fn, nfile, keep))
    frames = 0 if lab is None else lab.frames
    return resXH, lab, fit, dt, V, i0, frames, kept


def main():
    parser = build_parser()
    args = parser.parse_args()
    if args.bDoCrossCt and args.pairs_fn is None:
        parser.error('--crossCt needs --pairs FILE')
    if args.bDoDipolarCrossCt and args.pairs_fn is None:
        parser.error('--dipolarCrossCt needs --pairs FILE')
    if args.bDoDipolarCrossCt and args.tau is None:
        parser.error('--dipolarCrossCt needs --tau: the functions are block averages over the memory time')
    if args.bDoDipolarCrossCt and not all(f.endswith('.npy') or f.endswith('.npz') for f in args.infn):
        print("= = = ERROR: --dipolarCrossCt works on vector-file input (.npy/.npz), not on MDTraj input: the streaming front end keeps no "
              "distances.", file=sys.stderr)
        sys.exit(1)
    if args.bDoDipolarCt and args.tau is None:
        print("= = = Refusing to do dipolar correlation analysis without using a block averaging over memory_time tau!", file=sys.stderr)
        sys.exit(1)
    if args.bDoDipolarCt and not all(f.endswith('.npy') or f.endswith('.npz') for f in args.infn):
        print("= = = ERROR: --dipolarCt works on vector-file input (.npy/.npz), not on MDTraj input: the streaming front end keeps no "
              "distances.", file=sys.stderr)
        sys.exit(1)
    check_noe_lag_args(args)
    check_noesy_args(args)
    check_mode_args(args)
    time_start = time.time()
    rank, world = srdist.start()
    if args.bDoModeCt and world > 1:
        # the ranks hold ranges of vectors; the output is not sharded
        print("= = = ERROR: --modeCt does not run under torchrun with more than one rank; run it as a single process.", file=sys.stderr)
        sys.exit(1)
    if args.bDoDipolarCt and world > 1:
        # the ranks hold ranges of vectors; the distances and the output are not sharded
        print("= = = ERROR: --dipolarCt does not run under torchrun with more than one rank; run it as a single process.", file=sys.stderr)
        sys.exit(1)
    if args.bDoDipolarCrossCt and world > 1:
        # the ranks hold ranges of vectors and a pair needs both of its vectors; the distances and the output are not sharded
        print("= = = ERROR: --dipolarCrossCt needs all vectors on one GPU and does not run under torchrun with more than one rank; "
              "run it as a single process.", file=sys.stderr)
        sys.exit(1)
    if args.help_sel:
        print("Notes: This program uses MDTraj selection syntax, e.g. 'chain A and resname GLY and name HA1 HA2'.")
        sys.exit(0)
    tau_memory = args.tau
    if args.bDoCt and tau_memory is None:
        print("= = = Refusing to do C(t)-analysis without using a block averaging over memory_time tau!", file=sys.stderr)
        sys.exit(1)
    if args.bDoCrossCt and tau_memory is None:
        print("= = = Refusing to do cross-correlation analysis without using a block averaging over memory_time tau!", file=sys.stderr)
        sys.exit(1)
    if args.bDoCrossCt and world > 1:
        # the ranks hold ranges of vectors and a pair needs both of its vectors
        print("= = = ERROR: --crossCt needs all vectors on one GPU and does not run under torchrun with more than one rank; "
              "run it as a single process.", file=sys.stderr)
        sys.exit(1)
    bDoVecDistrib = args.bDoVecDistrib or args.bDoVecHist
    q_rot = None
    if args.vecRotQ != '':
        q_rot = np.array([float(v) for v in args.vecRotQ.split()])
        if len(q_rot) != 4 or not np.allclose(np.dot(q_rot, q_rot), 1):
            print("= = = ERROR: input rotation quaternion is malformed!", q_rot)
            sys.exit(23)
    if args.bDoIREDCt and not args.bDoIRED:
        print("= = = ERROR: --iRED_Ct extends --iRED and needs it; give both.", file=sys.stderr)
        sys.exit(1)
    if args.bDoIRED and world > 1:
        # the ranks hold ranges of vectors and the matrix needs every pair
        print("= = = ERROR: --iRED needs all vectors on one GPU and does not run under torchrun with more than one rank; "
              "run it as a single process.", file=sys.stderr)
        sys.exit(1)
    if len(args.topfn) > 1 and len(args.topfn) != len(args.infn):
        print("= = ERROR: When giving multiple reference files, you must have one for each trajecfile file given!", file=sys.stderr)
        sys.exit(1)
    if args.noe_cutoff is not None and not args.bDoNoeMap:
        print("= = = ERROR: --noeCutoff belongs to --noeMap; give both.", file=sys.stderr)
        sys.exit(1)
    if args.bDoNoeMap:
        if world > 1:
            # the tile pairs are not sharded over ranks
            print("= = = ERROR: --noeMap does not run under torchrun with more than one rank; run it as a single process.", file=sys.stderr)
            sys.exit(1)
        if not run_noe_map(args, srdist.output_prefix(args.out_pref)):
            # a file of `indexP` alone holds no bonds: nothing else to analyse
            print("= = Finished. Total seconds elapsed: %g" % (time.time() - time_start))
            srdist.finish()
            return

    def frames_per_chunk_of(dt):
        if tau_memory is None:
            return None
        if dt > 0.5 * tau_memory:
            print("= = = ERROR: delta-t form the trajectory is too small relative to tau! %g vs. %g" % (dt, tau_memory), file=sys.stderr)
            sys.exit(1)
        return int(tau_memory / dt)

    host_fit = host_lab = None   # host copies of the vectors (vector-file input only: the --vecDist listing and the chunk-sharded C(t) need them)
    if all(f.endswith('.npy') or f.endswith('.npz') for f in args.infn):
        resXH, vecXH, vecXHfit, deltaT = load_vector_files(args.infn, args.dt)
        if args.qfile is not None:
            from spinrelax_amd import plumedcolvario
            if len(args.qfile) != len(vecXH):
                print("= = = ERROR: --qfile needs one orientation file per trajectory file!", file=sys.stderr)
                sys.exit(1)
            print("= = = De-tumbling the lab-frame vectors with the per-frame orientation quaternions.")
            vecXHfit = []
            for fn, lab in zip(args.qfile, vecXH):
                _, q = plumedcolvario.read_qorient(fn)
                if q.shape[0] != lab.shape[0]:
                    print("= = = ERROR: %s holds %i frames, the trajectory %i!" % (fn, q.shape[0], lab.shape[0]), file=sys.stderr)
                    sys.exit(1)
                vecXHfit.append(hostct.detumble_vectors(lab, q))
        F = frames_per_chunk_of(deltaT)
        # ONE upload per vector set, of this rank's columns only; when the file holds no separate lab-frame vectors the two
        # sets are the same arrays and share the resident copy
        same = all(a is b for a, b in zip(vecXH, vecXHfit)) and len(vecXH) == len(vecXHfit)
        # fewer vectors than ranks: C(t) is sharded over the replicate chunks instead; the vector
        # distribution keeps the vector sharding (the surplus ranks idle there)
        repl = args.bDoCt and srdist.replicate_sharding(vecXHfit[0].shape[1])
        rv_fit, V, i0, N = hostct.upload_shard(vecXHfit, F)
        rv_lab = rv_fit if same or not args.bDoCt or repl else hostct.upload_shard(vecXH, F)[0]
        host_fit, host_lab = vecXHfit, vecXH
        frames_per_file = [v.shape[0] if F is None else (v.shape[0] // F) * F for v in vecXH]      # what upload_shard kept
        del vecXH
    else:
        if args.qfile is not None:
            print("= = = ERROR: --qfile works on vector-file input (.npy/.npz), not on MDTraj input.", file=sys.stderr)
            sys.exit(1)
        resXH, rv_lab, rv_fit, deltaT, V, i0, N, frames_per_file = load_mdtraj(args, frames_per_chunk_of)
        repl = False
        if srdist.replicate_sharding(V):
            print("= = = ERROR: %i ranks for %i vectors: trajectory input is sharded by vector; use at most %i ranks (vector-file "
                  "input can shard the replicate chunks instead)." % (srdist.world(), V, V), file=sys.stderr)
            sys.exit(1)
        F = frames_per_chunk_of(deltaT)
        if N < 1:
            print("= = = ERROR: no trajectory holds a full block of memory time tau!", file=sys.stderr)
            sys.exit(1)
    print("= = Loading finished.")
    out_pref = srdist.output_prefix(args.out_pref)

    if tau_memory is not None:
        print("= = Reformatting all vecXH information into chunks of tau ( %g ) " % tau_memory)
        print("    ...debug: Using %i frames per chunk based on tau/dt (%g/%g)." % (F, tau_memory, deltaT))
        R = N // F

    if args.bDoCt:
        mode = 1 if args.exact else 0
        dt = hostct.calculate_dt(deltaT, tau_memory)
        print("= = = Conducting Ct_external using Palmer's approach.")
        print("= = = timestep: ", deltaT, "ps")
        print("= = = tau_memory: ", tau_memory, "ps")
        if repl:
            Ct, dCt = hostct.calculate_Ct_chunk_sharded(host_lab, F, mode=mode)
        else:
            Ct, dCt = hostct.calculate_Ct_resident(rv_lab, V, R, F, mode=mode)
        gs.print_sxylist(out_pref + '_Ctext.dat', resXH, dt, np.stack((Ct.T, dCt.T), axis=-1))
        print("= = = Conducting Ct_internal using Palmer's approach.")
        if repl:
            if not same:
                Ct, dCt = hostct.calculate_Ct_chunk_sharded(host_fit, F, mode=mode)
        elif rv_fit is not rv_lab:
            Ct, dCt = hostct.calculate_Ct_resident(rv_fit, V, R, F, mode=mode)
        gs.print_sxylist(out_pref + '_Ctint.dat', resXH, dt, np.stack((Ct.T, dCt.T), axis=-1))
    if args.bDoIRED:
        # the lab-frame vectors as they are held (P2(u_i.u_j) at equal times does not change under a rotation of the frame):
        # no superposition, no de-tumbling, no fit
        from spinrelax_amd import ired
        print("= = = Conducting iRED analysis of the %i vectors with %i global modes." % (V, args.ired_modes))
        if V <= args.ired_modes:
            print("= = = ERROR: iRED needs more vectors (%i) than global modes (%i)!" % (V, args.ired_modes), file=sys.stderr)
            sys.exit(1)
        try:
            if args.bDoIREDCt:
                res = ired.calculate_iRED_resident(rv_lab, frames_per_file, deltaT, window=args.ired_window, tau=tau_memory,
                                                   n_global=args.ired_modes, mode_ct=True)
            else:
                res = ired.calculate_iRED_resident(rv_lab, frames_per_file, deltaT, window=args.ired_window, tau=tau_memory,
                                                   n_global=args.ired_modes)
        except ValueError as exc:
            print("= = = ERROR: %s" % exc, file=sys.stderr)
            sys.exit(1)
        print("    ...%i windows of %i to %i frames." % (res['win_len'].size, res['win_len'].min(), res['win_len'].max()))
        gs.print_xylist(out_pref + '_iRED_S2.dat', resXH, np.stack((res['S2'], res['dS2'])) * args.zeta, True)
        gs.print_xylist(out_pref + '_iRED_eig.dat', np.arange(1, V + 1), res['eig'][np.newaxis, :], True)
        if args.bDoIREDCt:
            # lag k of the arrays is k frames: _Ctint.dat's layout (lags 1 .. F_w / 2, x = k dt) for the vectors, lag 0 too for the modes
            lags = np.arange(res['Cm'].shape[1]) * float(deltaT)
            gs.print_sxylist(out_pref + '_iRED_Ctint.dat', resXH, lags[1:], np.stack((res['Ct_vec'][1:].T, res['dCt_vec'][1:].T), axis=-1))
            _, dCm = ired.ired_reduce(res['Cm_w'].reshape(res['Cm_w'].shape[0], -1))
            gs.print_sxylist(out_pref + '_iRED_modeCt.dat', list(range(1, V + 1)), lags,
                             np.stack((res['Cm'], dCm.reshape(res['Cm'].shape)), axis=-1))
            gs.print_xylist(out_pref + '_iRED_tau.dat', np.arange(1, V + 1), np.stack((res['eig'], res['tau'])), True)
        if args.binary:
            extra = dict(Cm_w=res['Cm_w'], modes_w=res['modes_w']) if args.bDoIREDCt else {}
            np.savez(out_pref + '_iRED_matrix.npz', M=res['M'], win_start=res['win_start'], win_len=res['win_len'],
                     resid=np.array(resXH), **extra)
        print("      ...complete.")
    if rv_lab is not None and rv_lab is not rv_fit:
        rv_lab.close()
    if args.bDoCrossCt:
        try:
            pairs = hostct.read_pairs(args.pairs_fn, V)
        except (OSError, ValueError) as exc:
            print("= = = ERROR: %s" % exc, file=sys.stderr)
            sys.exit(1)
        if args.bCrossAsym:
            pairs = np.stack((pairs, pairs[:, ::-1]), axis=1).reshape(-1, 2)      # (i, j) then (j, i)
        print("= = = Conducting cross-correlation analysis of %i pairs of fitted vectors using Palmer's approach." % len(pairs))
        P0, dP0, Cx, dCx = hostct.calculate_Ct_cross_resident(rv_fit, pairs, R, F, symmetric=not args.bCrossAsym, mode=1 if args.exact else 0,
                                                              want_dP0=True)
        ordinals = list(range(1, len(pairs) + 1))
        gs.print_sxylist(out_pref + '_crossCtint.dat', ordinals, hostct.calculate_dt(deltaT, tau_memory), np.stack((Cx.T, dCx.T), axis=-1))
        with open(out_pref + '_crossPairs.dat', 'w') as fp:
            print("# pair i j resid_i resid_j P0 dP0", file=fp)
            for n, (i, j) in enumerate(pairs):
                print("%d %d %d %s %s %.8g %.8g" % (ordinals[n], i, j, resXH[i], resXH[j], P0[n], dP0[n]), file=fp)
        print("      ...complete.")
    if args.bDoDipolarCt:
        print("= = = Conducting distance-weighted dipolar correlation analysis of the fitted vectors using Palmer's approach.")
        try:
            dist = load_distance_files(args.infn, F)
            Cd, dCd, reff6, reff3, S2rad = hostct.calculate_Ct_dipolar_resident(rv_fit, R, F, dist=dist, mode=1 if args.exact else 0)
        except (ValueError, hostct.hip.SpinRelaxHipError) as exc:      # a bad distance, a zero-length vector, a chunk beyond both forms
            print("= = = ERROR: %s" % exc, file=sys.stderr)
            sys.exit(1)
        gs.print_sxylist(out_pref + '_dipolarCtint.dat', resXH, hostct.calculate_dt(deltaT, tau_memory), np.stack((Cd.T, dCd.T), axis=-1))
        with open(out_pref + '_dipolarDist.dat', 'w') as fp:
            print("# resid reff6 reff3 S2rad", file=fp)
            for n in range(V):
                print("%s %.8g %.8g %.8g" % (resXH[n], reff6[n], reff3[n], S2rad[n]), file=fp)
        print("      ...complete.")
    if args.bDoDipolarCrossCt:
        try:
            pairs = hostct.read_pairs(args.pairs_fn, V)
        except (OSError, ValueError) as exc:
            print("= = = ERROR: %s" % exc, file=sys.stderr)
            sys.exit(1)
        if args.bCrossAsym:
            pairs = np.stack((pairs, pairs[:, ::-1]), axis=1).reshape(-1, 2)      # (i, j) then (j, i)
        print("= = = Conducting distance-weighted cross-correlation analysis of %i pairs of fitted vectors using Palmer's approach." % len(pairs))
        try:
            dist = load_distance_files(args.infn, F)
            P0, dP0, Cx, dCx, reff6 = hostct.calculate_Ct_dipolar_cross_resident(rv_fit, pairs, R, F, dist=dist, symmetric=not args.bCrossAsym,
                                                                                 mode=1 if args.exact else 0)
        except (ValueError, hostct.hip.SpinRelaxHipError) as exc:      # a bad distance, a zero-length vector, a chunk beyond both forms
            print("= = = ERROR: %s" % exc, file=sys.stderr)
            sys.exit(1)
        ordinals = list(range(1, len(pairs) + 1))
        gs.print_sxylist(out_pref + '_dipolarCrossCtint.dat', ordinals, hostct.calculate_dt(deltaT, tau_memory), np.stack((Cx.T, dCx.T), axis=-1))
        with open(out_pref + '_dipolarCrossPairs.dat', 'w') as fp:
            print("# pair i j resid_i resid_j P0 dP0 reff6_i reff6_j", file=fp)
            for n, (i, j) in enumerate(pairs):
                print("%d %d %d %s %s %.8g %.8g %.8g %.8g" % (ordinals[n], i, j, resXH[i], resXH[j], P0[n], dP0[n], reff6[n, 0], reff6[n, 1]),
                      file=fp)
        print("      ...complete.")

    if args.bDoModeCt:
        run_mode_ct(args, out_pref, rv_fit, resXH, R, F, deltaT, q_rot)

    need_dist = args.bDoVecAverage or args.bDoS2 or (bDoVecDistrib and args.bDoVecHist)
    if need_dist:
        if q_rot is not None:
            print("= = = Rotating all fitted vectors by the input quaternion into PAF.")
        dist = hostct.vector_distribution_resident(rv_fit, V, N, q_rot, histBinX=args.histBin,
                                                   delta_t=deltaT if tau_memory is not None else -1,
                                                   tau_memory=tau_memory if tau_memory is not None else -1)
    if bDoVecDistrib and not args.bDoVecHist:
        # the full (phi, theta) listing needs every rotated vector on the host
        if host_fit is not None:
            used = [v[: (v.shape[0] // F) * F] if tau_memory is not None else v for v in host_fit]
            vec3d = used[0] if len(used) == 1 else np.concatenate(used, axis=0)
        else:
            part = rv_fit.download() if rv_fit is not None else np.empty((N, 0, 3), dtype=np.float32)
            vec3d = srdist.gather_rows(part, V, axis=1) if srdist.world() > 1 else part
    if rv_fit is not None:
        rv_fit.close()
    if args.bDoVecAverage:
        gs.print_xylist(out_pref + '_avgvec.dat', resXH, np.array(dist['avgvec']).T, True)
    if bDoVecDistrib:
        print("= = = Converting vectors into spherical coordinates.")
        if not args.bDoVecHist:
            # full (phi, theta) listing: rotation on the GPU, the two angle maps are plain numpy ufuncs
            rot = hostct.rotate_vector_simd(vec3d, q_rot) if q_rot is not None else vec3d
            r = np.linalg.norm(rot, axis=-1)
            pt = np.stack((np.arctan2(rot[..., 1], rot[..., 0]), np.arccos(rot[..., 2] / r)), axis=-1)
            pt = np.transpose(pt, axes=(1, 0, 2))
            if args.binary:
                gs.save_vecPhiTheta_npz(out_pref + '_vecPhiTheta.npz', resXH, pt)
            else:
                rtp = np.concatenate((np.transpose(r)[..., None], pt), axis=-1)
                gs.print_s3d(out_pref + '_vecPhiTheta.dat', resXH, rtp, (1, 2))
        else:
            print("= = = Histgrams will use Lambert Cylindrical projection by converting Theta spanning (0,pi) to cos(Theta) spanning (-1,1)")
            if args.binary:
                gs.save_vecHistogram_npz(out_pref + '_vecHistogram.npz', resXH, dist['hist'], dist['edges'])
            else:
                for i in range(len(resXH)):
                    ofile = out_pref + '_vecXH_' + str(resXH[i]) + '.hist'
                    gs.print_gplot_hist(ofile, dist['hist'][i], dist['edges'],
                                        header='# Lamber Cylindrical Histogram over phi,cos(theta).', bSphere=True)
                    print("= = = Written to output: ", ofile)
    if args.bDoS2:
        if tau_memory is not None:
            print("= = = Conducting S2 analysis using memory time to chop input-trajectories", tau_memory, "ps")
        else:
            print("= = = Conducting S2 analysis directly from trajectories.")
        S2 = dist['S2']
        gs.print_xylist(out_pref + '_S2.dat', resXH, (S2.T) * args.zeta, True)
        print("      ...complete.")
    print("= = Finished. Total seconds elapsed: %g" % (time.time() - time_start))
    srdist.finish()


if __name__ == '__main__':
    main()
