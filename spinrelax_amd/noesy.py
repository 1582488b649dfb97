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

A per-pair tau_e comes from the map itself when it was made with lags (noe.dipolar_map(..., lags=...), csrc/sr_noe_lagged.hip):
tau_e='map' takes map_result['tau_e'], in seconds, floored at TAU_E_FLOOR.

Not done: anisotropic tumbling (the map keeps no pair orientation in the diffusion frame), other nuclei than protons, more than one GPU.
"""
import numpy as np

from . import hip
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


def _tau_e(map_result, tau_e):
    """tau_e as the library takes it: a scalar or one value per pair in seconds; 'map': map_tau_e(map_result)"""
    if not isinstance(tau_e, str):
        return tau_e
    if tau_e != 'map':
        raise ValueError("tau_e must be a time in seconds, one per pair, or 'map'")
    return map_tau_e(map_result)


def _rates_dev(c, map_result, field_MHz, tau_c, tau_e, leak, unit):
    """R as a torch tensor on the context's device"""
    P = _n_spins(map_result)
    tau_e = _tau_e(map_result, tau_e)
    torch, dev = _torch_dev(c)
    R_d = torch.empty((P, P), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    c.noesy_rates_dev(map_result['A6'], map_result['S2'], P, omega_H(field_MHz), tau_c, tau_e, leak, prefactor(unit), R_d.data_ptr())
    return R_d


def rate_matrix(map_result, field_MHz, tau_c, tau_e=1e-10, leak=0.0, unit='nm', ctx=None):
    """R (P, P) float64 of the P spins of a map: noe.dipolar_map's dict, or anything that holds A6, S2 (P (P - 1) / 2 each, pairs in
    the order of noe.pair_index) and index (P).  field_MHz: the proton frequency; tau_c, tau_e in seconds, tau_e a scalar or one value
    per pair, or 'map': the map's own tau_e (a map made with lags and dt in seconds per frame), floored at TAU_E_FLOOR; leak in 1 / s, a
    scalar or one value per spin; unit: the unit of the coordinates the map was taken from, 'nm' (MDTraj's,
    the default), 'A', or metres per unit.  R_ij = sigma_ij, R_ii = sum_j rho_ij + leak_i, exactly symmetric."""
    tau_e = _tau_e(map_result, tau_e)           # a map without tau_e is refused before a context is asked for
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


def noesy(map_result, mixing_times, field_MHz, tau_c, tau_e=1e-10, leak=0.0, unit='nm', ctx=None):
    """rate_matrix and intensities in one go, R staying on the device between the two.  Returns dict(R (P, P), sigma (npairs) the
    cross-relaxation rates in the map's pair order, rho (P) the auto-relaxation rates R_ii (leak included), A (n_tau, P, P),
    mixing_times, index, pairs)."""
    tau_e = _tau_e(map_result, tau_e)           # a map without tau_e is refused before a context is asked for
    c = _ctx(ctx)
    tau = _mixing(mixing_times)
    R_d = _rates_dev(c, map_result, field_MHz, tau_c, tau_e, leak, unit)
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
