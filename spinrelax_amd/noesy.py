"""
NOESY cross-peak intensities from the all-pairs dipolar map (noe.dipolar_map) by the full relaxation matrix, spin diffusion included
(Macura & Ernst, Mol. Phys. 41, 95 (1980); Keepers & James, J. Magn. Reson. 57, 404 (1984), CORMA; the model-free rates from <r^-6> and
S2: Brueschweiler et al., J. Am. Chem. Soc. 114, 2289 (1992)).

With A6 = <r^-6> and S2 of a pair from the map, isotropic tumbling with correlation time tau_c, internal motion with tau_e and
1 / t' = 1 / tau_c + 1 / tau_e:

    J(w)     = S2 tau_c / (1 + w^2 tau_c^2) + (1 - S2) t' / (1 + w^2 t'^2)
    sigma_ij = q A6 [6 J(2 w_H) - J(0)]                        (cross-relaxation rate, R_ij)
    rho_ij   = q A6 [J(0) + 3 J(w_H) + 6 J(2 w_H)]             (R_ii = sum_j rho_ij + leak_i)
    A(tau_m) = exp(-R tau_m)                                   (A_ij: the cross peak of i and j per unit of equilibrium magnetisation)

q = 0.1 (mu0 / 4 pi)^2 hbar^2 gamma_H^4 / u^6 with u the length of one coordinate unit in metres.  The rate matrix and the exponential
are computed on the MI355X (csrc/sr_noesy.hip) and nowhere else: without a GPU every function that needs them raises SpinRelaxHipError.
sum_groups, write_noesy and read_noesy are host numpy.

A per-pair tau_e comes from the map itself when it was made with lags (noe.dipolar_map(..., lags=...), csrc/sr_noe.hip):
tau_e='map' takes map_result['tau_e'], in seconds, floored at TAU_E_FLOOR.

Anisotropic tumbling: with D = (Dx, Dy, Dz) in 1 / s in the place of tau_c, and a map made with modes=True in the tensor's
principal-axis frame (noe.dipolar_map(..., modes=True, frame=q_F), csrc/sr_noe.hip), the five rates E_m of the tensor
(_hostmath.D_coefficients_ellipsoid) and per pair the mode amplitudes a_m (lag 0) and plateaus c_m (noe.mode_amplitudes,
noe.mode_plateau; sum_m a_m = A6, sum_m c_m = S2 A6), g(x, y) = x / (x^2 + y^2):

    J(w)     = sum_m [ c_m g(E_m, w) + max(a_m - c_m, 0) g(E_m + 1 / tau_e, w) ]
    sigma_ij = q [6 J(2 w_H) - J(0)]      rho_ij = q [J(0) + 3 J(w_H) + 6 J(2 w_H)]

With Dx = Dy = Dz = 1 / (6 tau_c) this is the formula above.  tau_e='modes': every mode of every pair with its own tau_e (noe.mode_tau_e).

Not done: other nuclei than protons, more than one GPU.
"""
import numpy as np

from . import hip, noe
from ._hostmath import D_coefficients_ellipsoid
from .noe import n_pairs, pair_list
from .spectral_densities import GAMMA

# 0.1 (mu0 / 4 pi)^2 hbar^2 gamma_H^4 in SI units (m^6 s^-2): the constant of relaxationExperiment.get_f_DD with both spins 1H
Q_HH = 0.10 * 1.1121216813552401e-82 * GAMMA['1H'] ** 4.0
UNITS = {'nm': 1e-9, 'A': 1e-10}
# tau_e='map': the smallest internal correlation time handed to the library, in seconds.  The library needs tau_e > 0, the map gives 0
# for a rigid pair and for one whose C_dd is at its plateau by the first lag; at 1 ps the internal term (1 - S2) t' is negligible
# beside S2 tau_c of any molecule that gives a NOESY spectrum (tau_c of nanoseconds).
TAU_E_FLOOR = 1e-12


def _ctx(ctx):
    return ctx if ctx is not None else hip.default_context()


def prefactor(unit='nm'):
    """q / u^6 in (coordinate unit)^6 s^-2; unit 'nm', 'A' or the length of one coordinate unit in metres"""
    u = UNITS[unit] if isinstance(unit, str) else float(unit)
    return Q_HH * u ** -6.0


def omega_H(field_MHz):
    """proton Larmor frequency in rad / s from the spectrometer's proton frequency in MHz"""
    return 2.0 * np.pi * float(field_MHz) * 1e6


def _n_spins(map_result):
    return int(np.asarray(map_result['index']).size)


def _torch_dev(c):
    import torch
    return torch, torch.device('cuda', c.device)


def map_tau_e(map_result):
    """the per-pair tau_e of a map made with lags as the rate matrix takes it: map_result['tau_e'], which must be in seconds
    (noe.dipolar_map(..., lags=..., dt=<seconds per frame>)), floored at TAU_E_FLOOR; ValueError for a map without tau_e"""
    if 'tau_e' not in map_result:
        raise ValueError("tau_e='map' needs a map made with lags (noe.dipolar_map(..., lags=...)): this one holds no tau_e")
    return np.maximum(np.asarray(map_result['tau_e'], dtype=np.float64), TAU_E_FLOOR)


def _tau_e(map_result, tau_e, D=None):
    """tau_e as the library takes it: a scalar or one value per pair in seconds; 'map': map_tau_e(map_result); with D also one value
    per pair and mode, or 'modes': mode_tau_e(map_result, D)"""
    if not isinstance(tau_e, str):
        return tau_e
    if tau_e == 'modes' and D is not None:
        return mode_tau_e(map_result, D)
    if tau_e != 'map':
        raise ValueError("tau_e must be a time in seconds, one per pair, or 'map'" + (" or 'modes'" if D is not None else ''))
    return map_tau_e(map_result)


def mode_tau_e(map_result, D):
    """the per-pair, per-mode tau_e (npairs, 5) of a map made with modes=True, lags beyond 0 and dt in seconds per frame as the rate
    matrix takes it: noe.mode_tau_e, floored at TAU_E_FLOOR (a mode whose a_m - c_m is not positive gets the floor)"""
    return np.maximum(noe.mode_tau_e(map_result, D), TAU_E_FLOOR)


def _check_tumbling(map_result, tau_c, D):
    """tau_c or D, not both; with D the map must hold the mode sums.  ValueError before a context is asked for"""
    if D is None:
        if tau_c is None:
            raise ValueError('give the overall correlation time tau_c, or the diffusion tensor D = (Dx, Dy, Dz)')
        return None
    if tau_c is not None:
        raise ValueError('tau_c and D both describe the tumbling; with D, tau_c must be None')
    D = np.asarray(D, dtype=np.float64)
    if D.shape != (3,) or not np.all(np.isfinite(D)) or np.any(D <= 0):
        raise ValueError('D must be (Dx, Dy, Dz) in 1 / s, finite and > 0')
    if 'H' not in map_result:
        raise ValueError('D needs a map made with modes=True (noe.dipolar_map(..., modes=True, frame=...)): this one holds no H')
    return D


def mode_inputs(map_result, D):
    """(a, c, E) as the library takes them: a (npairs, 5) = noe.mode_amplitudes of the map's H at lag 0, c (npairs, 5) =
    noe.mode_plateau of its mean tensor in its frame, E (5) the tensor's rates.  Rounding is taken out as S2 is clipped in the
    isotropic form: a below 0 becomes 0, c is clipped to [0, a] (exactly, c_m <= a_m: a squared mean is below the mean square)."""
    a = np.maximum(noe.mode_amplitudes(np.asarray(map_result['H'])[0], D), 0.0)
    c = np.clip(noe.mode_plateau(map_result['T'], D, map_result.get('frame')), 0.0, a)
    return a, c, D_coefficients_ellipsoid(D)


def _rates_dev(c, map_result, field_MHz, tau_c, tau_e, leak, unit, D=None):
    """R as a torch tensor on the context's device"""
    P = _n_spins(map_result)
    tau_e = _tau_e(map_result, tau_e, D)
    torch, dev = _torch_dev(c)
    R_d = torch.empty((P, P), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    if D is not None:
        a, cm, E = mode_inputs(map_result, D)
        c.noesy_rates_modes_dev(a, cm, E, P, omega_H(field_MHz), tau_e, leak, prefactor(unit), R_d.data_ptr())
    else:
        c.noesy_rates_dev(map_result['A6'], map_result['S2'], P, omega_H(field_MHz), tau_c, tau_e, leak, prefactor(unit), R_d.data_ptr())
    return R_d


def rate_matrix(map_result, field_MHz, tau_c=None, tau_e=1e-10, leak=0.0, unit='nm', ctx=None, D=None):
    """R (P, P) float64 of the P spins of a map: noe.dipolar_map's dict, or anything that holds A6, S2 (P (P - 1) / 2 each, pairs in
    the order of noe.pair_index) and index (P).  field_MHz: the proton frequency; tau_c, tau_e in seconds, tau_e a scalar or one value
    per pair, or 'map': the map's own tau_e (a map made with lags and dt in seconds per frame), floored at TAU_E_FLOOR; leak in 1 / s, a
    scalar or one value per spin; unit: the unit of the coordinates the map was taken from, 'nm' (MDTraj's,
    the default), 'A', or metres per unit.  R_ij = sigma_ij, R_ii = sum_j rho_ij + leak_i, exactly symmetric.
    D = (Dx, Dy, Dz) in 1 / s: anisotropic tumbling, in the place of tau_c (which must then be None), on a map made with modes=True in
    the tensor's principal-axis frame; tau_e may then also be one value per pair and mode (npairs, 5), or 'modes' (mode_tau_e)."""
    D = _check_tumbling(map_result, tau_c, D)
    tau_e = _tau_e(map_result, tau_e, D)        # a map without tau_e is refused before a context is asked for
    if D is not None:
        a, cm, E = mode_inputs(map_result, D)
        return _ctx(ctx).noesy_rates_modes(a, cm, E, _n_spins(map_result), omega_H(field_MHz), tau_e, leak, prefactor(unit))
    return _ctx(ctx).noesy_rates(map_result['A6'], map_result['S2'], _n_spins(map_result), omega_H(field_MHz), tau_c, tau_e, leak,
                                 prefactor(unit))


def _expm_dev(c, R_d, tau):
    torch, dev = _torch_dev(c)
    P = int(R_d.shape[0])
    c.symm_expm_check(P, tau.size)              # the library's refusal, with its sizes, before torch allocates
    A_d = torch.empty((tau.size, P, P), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)                 # the allocation is torch's, the kernels run on the context's stream
    c.symm_expm_dev(R_d.data_ptr(), P, tau, A_d.data_ptr())
    c.sync()
    return A_d


def _mixing(mixing_times):
    tau = np.ascontiguousarray(np.atleast_1d(mixing_times), dtype=np.float64)
    if tau.ndim != 1 or tau.size < 1:
        raise ValueError('mixing_times must be a non-empty list of times in seconds')
    return tau


def intensities(R, mixing_times, ctx=None):
    """A (n_tau, P, P) float64, A[k] = exp(-R mixing_times[k]), for a symmetric rate matrix R in 1 / s and mixing times in seconds.
    Each mixing time is computed from R on its own: A(tau) has the same bits alone and in a list."""
    c = _ctx(ctx)
    R = np.ascontiguousarray(R, dtype=np.float64)
    if R.ndim != 2 or R.shape[0] != R.shape[1]:
        raise ValueError('R must be square')
    tau = _mixing(mixing_times)
    torch, dev = _torch_dev(c)
    R_d = torch.from_numpy(R).to(dev)
    return _expm_dev(c, R_d, tau).cpu().numpy()


def noesy(map_result, mixing_times, field_MHz, tau_c=None, tau_e=1e-10, leak=0.0, unit='nm', ctx=None, D=None):
    """rate_matrix and intensities in one go, R staying on the device between the two.  Returns dict(R (P, P), sigma (npairs) the
    cross-relaxation rates in the map's pair order, rho (P) the auto-relaxation rates R_ii (leak included), A (n_tau, P, P),
    mixing_times, index, pairs).  tau_c or D, and tau_e: as in rate_matrix."""
    D = _check_tumbling(map_result, tau_c, D)
    tau_e = _tau_e(map_result, tau_e, D)        # a map without tau_e is refused before a context is asked for
    c = _ctx(ctx)
    tau = _mixing(mixing_times)
    R_d = _rates_dev(c, map_result, field_MHz, tau_c, tau_e, leak, unit, D)
    A = _expm_dev(c, R_d, tau).cpu().numpy()
    R = R_d.cpu().numpy()
    P = R.shape[0]
    pr = pair_list(P)
    return dict(R=R, sigma=R[pr[:, 0], pr[:, 1]], rho=np.diagonal(R).copy(), A=A, mixing_times=tau,
                index=np.asarray(map_result['index'], dtype=np.int64), pairs=pr)


def sum_groups(A, groups):
    """A_GH = sum_{i in G, j in H} A_ij for groups of equivalent or unresolved spins (methyls, flipping rings): A (..., P, P), groups a
    list of lists of positions 0 .. P - 1, each position in at most one group -> (..., n_groups, n_groups).  A trajectory carries every
    proton explicitly, so the sum is all that equivalence needs."""
    A = np.asarray(A, dtype=np.float64)
    if A.ndim < 2 or A.shape[-1] != A.shape[-2]:
        raise ValueError('A must be (..., P, P)')
    P = A.shape[-1]
    M = np.zeros((len(groups), P))
    seen = np.zeros(P, dtype=bool)
    for g, members in enumerate(groups):
        m = np.asarray(members, dtype=np.int64).ravel()
        if m.size < 1:
            raise ValueError('group %d is empty' % g)
        if m.min() < 0 or m.max() >= P:
            raise ValueError('group %d holds a position outside the %d spins' % (g, P))
        if np.unique(m).size != m.size or seen[m].any():
            raise ValueError('position listed twice (group %d)' % g)
        seen[m] = True
        M[g, m] = 1.0
    return M @ A @ M.T


def read_groups(path):
    """a groups file: one group per line, white-space separated positions in the list of selected spins; # starts a comment"""
    groups = []
    with open(path) as fp:
        for line in fp:
            line = line.split('#', 1)[0].split()
            if line:
                groups.append([int(w) for w in line])
    return groups


def _columns(n_tau):
    return ['i', 'j', 'name_i', 'name_j', 'sigma'] + ['A%d' % k for k in range(n_tau)]


def write_noesy(path, result, names=None, reff6=None, cutoff=None):
    """<o>_noesy.dat: a header '# i j name_i name_j sigma A0 A1 ...', a line '# mixing_times t0 t1 ...' (seconds, %.8g), then one row
    per diagonal i = j (sigma column: R_ii) and per pair i < j, row-major: the atom indices, the names, sigma and one %.8g column per
    mixing time.  cutoff keeps the pairs with reff6 <= cutoff (reff6: the map's, in the pair order; the diagonal rows always stay).
    names: one per spin, default the atom index.  Returns the number of rows."""
    idx = np.asarray(result['index'], dtype=np.int64)
    P = idx.size
    A, R, tau = np.asarray(result['A']), np.asarray(result['R']), np.asarray(result['mixing_times'], dtype=np.float64)
    if A.shape != (tau.size, P, P) or R.shape != (P, P):
        raise ValueError('result must hold A (n_tau, P, P) and R (P, P) of the P = %d spins of index' % P)
    names = [str(a) for a in idx] if names is None else [str(n) for n in names]
    if len(names) != P:
        raise ValueError('names must give one name per selected atom')
    if any((not n) or any(ch.isspace() for ch in n) for n in names):
        raise ValueError('names must be non-empty and free of white space')
    keep = None
    if cutoff is not None:
        if reff6 is None or np.asarray(reff6).shape != (n_pairs(P),):
            raise ValueError('a cutoff needs reff6, one value per pair')
        keep = np.asarray(reff6) <= cutoff
    rows = 0
    with open(path, 'w') as fp:
        fp.write('# ' + ' '.join(_columns(tau.size)) + '\n')
        fp.write('# mixing_times ' + ' '.join('%.8g' % t for t in tau) + '\n')
        k = 0
        for i in range(P):
            for j in range(i, P):
                if j > i:
                    k += 1
                    if keep is not None and not keep[k - 1]:
                        continue
                fp.write('%d %d %s %s %.8g %s\n' % (idx[i], idx[j], names[i], names[j], R[i, j], ' '.join('%.8g' % a for a in A[:, i, j])))
                rows += 1
    return rows


def read_noesy(path):
    """parse write_noesy's file back: dict(i, j int64, name_i, name_j lists of str, sigma (rows) float64, A (rows, n_tau) float64,
    mixing_times (n_tau) float64)"""
    tau = None
    i, j, ni, nj, sig, A = [], [], [], [], [], []
    with open(path) as fp:
        for line in fp:
            if line.startswith('# mixing_times'):
                tau = np.array(line.split()[2:], dtype=np.float64)
                continue
            if line.startswith('#') or not line.strip():
                continue
            w = line.split()
            if tau is None or len(w) != 5 + tau.size:
                raise ValueError('%s: a row with %d columns, expected %s' % (path, len(w), 'a mixing_times line first' if tau is None else 5 + tau.size))
            i.append(w[0]); j.append(w[1]); ni.append(w[2]); nj.append(w[3]); sig.append(w[4]); A.append(w[5:])
    if tau is None:
        raise ValueError('%s: no mixing_times line' % path)
    return dict(i=np.array(i, dtype=np.int64), j=np.array(j, dtype=np.int64), name_i=ni, name_j=nj, sigma=np.array(sig, dtype=np.float64),
                A=np.array(A, dtype=np.float64).reshape(len(i), tau.size), mixing_times=tau)
