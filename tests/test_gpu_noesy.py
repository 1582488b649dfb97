"""
GPU tests of the NOESY layer (csrc/sr_noesy.hip, spinrelax_amd/noesy.py) against the CPU definitions of tests/noesy_oracle.py.

Bars.  u = 2^-53.
  product      |C - A B|_ij <= 2 P u (|A| |B|)_ij: the textbook bound of a length-P inner product in float64 (P u each for the kernel
               and for numpy's reference), whatever the order of summation.
  sigma        64 u q A6 (J(0) + 6 J(2w)): relative to the sum of magnitudes, because sigma crosses zero near w tau_c = 1.12.
  R_ii         P u sum_j rho_ij (the sum) + 64 u R_ii (the terms).
  exponential  1e-12 absolute on entries in [-1, 1].  An emulation of exactly the library's algorithm (theta = 0.5, degree 12 by Horner,
               float64) in numpy on these inputs differs from scipy.linalg.expm and from the eigh form by at most 7e-15 for s <= 4 and
               2.0e-14 at P = 150, s = 8 (2.8e-14 at P = 400, s = 8; an earlier emulation on other draws gave up to 5e-14); the two CPU
               references differ by at most 1.1e-14.  1e-12 is 20 times that worst case; the margin pays for the matrix pipe's
               different summation order (measured on MI355X: 1.9e-14 and 2.0e-14 at P = 150, s = 8, the emulation's figures).  The
               test asserts through symm_expm_plan that its cases need s <= 8.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import noesy_oracle as oracle
from conftest import ROOT
from noesy_oracle import U53
from spinrelax_amd import hip, noe, noesy
from spinrelax_amd._lib import SpinRelaxHipError
from test_gpu_noe import make_body

pytestmark = pytest.mark.gpu

TAUS = (0.0, 0.05, 0.2, 0.8)
W = oracle.omega_H(oracle.FIELD)


@pytest.fixture(scope='module')
def ctx():
    c = hip.Context()
    yield c
    c.close()


def to_dev(ctx, a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order='C')).to(torch.device('cuda', ctx.device))


def symm_mul(ctx, A, B, alpha=1.0, beta=0.0):
    import torch
    A_d, B_d = to_dev(ctx, A), to_dev(ctx, B)
    C_d = torch.full_like(A_d, float('nan'))
    torch.cuda.synchronize()
    ctx.symm_mul_dev(A_d.data_ptr(), B_d.data_ptr(), A.shape[0], C_d.data_ptr(), alpha=alpha, beta=beta)
    ctx.sync()
    return C_d.cpu().numpy()


def defined_product(A, B, alpha, beta):
    """the documented result for any symmetric input: the tiles with tile row <= tile column of alpha A B + beta I (of a diagonal tile
    the entries i <= j), mirrored below"""
    P = A.shape[0]
    C = alpha * (A @ B) + beta * np.eye(P)
    i = np.arange(P)
    t = i // 64
    upper = (t[:, None] < t[None, :]) | ((t[:, None] == t[None, :]) & (i[:, None] <= i[None, :]))
    return np.where(upper, C, C.T)


@functools.lru_cache(maxsize=None)
def product_inputs(P):
    """A: symmetric, entries k / 2^20 with |k| < 2^20.  B = I + A / 2 + A A / 4 is then EXACT in float64 (A A: products of 40 bits, sums
    of at most 200 of them), so A and B commute exactly while A B itself rounds.  N: symmetric normal, does not commute with A."""
    rng = np.random.default_rng(100 + P)
    K = rng.integers(-2 ** 20 + 1, 2 ** 20, (P, P))
    A = np.triu(K) + np.triu(K, 1).T
    A = A / 2.0 ** 20
    B = np.eye(P) + A / 2 + (A @ A) / 4
    # exact: 2^42 B is the integer matrix 2^42 I + 2^21 K + K K (below 2^53), so B is a polynomial in A to the last bit
    KB = (A * 2.0 ** 20).astype(np.int64)
    KB = KB @ KB + 2 ** 21 * KB + 2 ** 42 * np.eye(P, dtype=np.int64)
    assert np.abs(KB).max() < 2 ** 53 and np.array_equal(B * 2.0 ** 42, KB.astype(np.float64)) and np.array_equal(B, B.T)
    N = rng.standard_normal((P, P))
    N = N + N.T
    for a in (A, B, N):
        a.setflags(write=False)
    return A, B, N


@pytest.mark.parametrize('P', [1, 2, 63, 64, 65, 129, 200])
def test_product_of_commuting_matrices(ctx, P):
    A, B, _ = product_inputs(P)
    C = symm_mul(ctx, A, B)
    ref, bound = A @ B, 2 * P * U53 * (np.abs(A) @ np.abs(B))
    err = np.abs(C - ref)
    print('P = %d: max |C - A B| / bound = %.3g' % (P, np.max(err / bound)))
    assert np.all(err <= bound)
    assert C.tobytes() == C.T.copy().tobytes()                     # symmetric bit for bit
    assert symm_mul(ctx, A, B).tobytes() == C.tobytes()            # and the same bits again
    # alpha and beta, and C written over an operand
    import torch
    A_d, B_d = to_dev(ctx, A), to_dev(ctx, B)
    torch.cuda.synchronize()
    ctx.symm_mul_dev(A_d.data_ptr(), B_d.data_ptr(), P, B_d.data_ptr(), alpha=0.5, beta=2.0)
    ctx.sync()
    C2 = B_d.cpu().numpy()
    assert np.array_equal(C2, 0.5 * C + 2.0 * np.eye(P))            # 0.5 C is exact, + 2 on the diagonal is one rounding, the same here


@pytest.mark.parametrize('P', [65, 200])
def test_product_definition_without_commutation(ctx, P):
    A, _, N = product_inputs(P)
    C = symm_mul(ctx, A, N, alpha=-1.5, beta=0.25)
    ref = defined_product(A, N, -1.5, 0.25)
    assert np.max(np.abs(ref - (-1.5 * (A @ N) + 0.25 * np.eye(P)))) > 1.0       # the mirror is not the product: the definition is what is tested
    bound = 1.5 * 2 * P * U53 * (np.abs(A) @ np.abs(N))
    bound = np.maximum(bound, bound.T) + 4 * U53 * np.abs(ref)
    assert np.all(np.abs(C - ref) <= bound)
    assert C.tobytes() == C.T.copy().tobytes()


# ---- rates ----
def rate_case(P, tc, per_pair):
    A6, S2, _ = oracle.synthetic(P)
    rng = np.random.default_rng(P)
    te = rng.uniform(2e-11, 2e-10, A6.size) if per_pair else oracle.TAU_E
    leak = rng.uniform(0.0, 1.0, P) if per_pair else oracle.LEAK
    return A6, S2, te, leak


@pytest.mark.parametrize('per_pair', [False, True])
@pytest.mark.parametrize('tc', oracle.TAU_C)
@pytest.mark.parametrize('P', [2, 47, 65])
def test_rates_against_numpy(ctx, P, tc, per_pair):
    A6, S2, te, leak = rate_case(P, tc, per_pair)
    R = ctx.noesy_rates(A6, S2, P, W, tc, te, leak, oracle.Q_ANGSTROM)
    ref, RHO, MAG = oracle.rate_matrix(A6, S2, P, W, tc, te, leak, oracle.Q_ANGSTROM)
    assert R.tobytes() == R.T.copy().tobytes()
    off = ~np.eye(P, dtype=bool)
    assert np.all(np.abs(R - ref)[off] <= 64 * U53 * MAG[off])
    d, dref = np.diagonal(R), np.diagonal(ref)
    assert np.all(np.abs(d - dref) <= P * U53 * RHO.sum(axis=1) + 64 * U53 * dref)
    sig = ref[off]
    assert (sig < 0).all() if tc == 5e-9 else (sig > 0).mean() > 0.9           # slow tumbling: negative; fast: positive for most pairs
    # the device-resident form gives the same bits
    import torch
    R_d = torch.empty((P, P), dtype=torch.float64, device=torch.device('cuda', ctx.device))
    torch.cuda.synchronize()
    ctx.noesy_rates_dev(A6, S2, P, W, tc, te, leak, oracle.Q_ANGSTROM, R_d.data_ptr())
    ctx.sync()
    assert R_d.cpu().numpy().tobytes() == R.tobytes()


def test_rates_closed_form_rigid_pair(ctx):
    """one rigid pair, S2 = 1, r = 2.5 A, 600 MHz, tau_c = 5 ns: tau_e drops out"""
    r, tc = 2.5, 5e-9
    q = 0.1 * 1.1121216813552401e-82 * 267.513e6 ** 4 / (r * 1e-10) ** 6
    w = 2 * np.pi * 600e6
    sigma = q * (6 * tc / (1 + 4 * w * w * tc * tc) - tc)
    rho = q * (tc + 3 * tc / (1 + w * w * tc * tc) + 6 * tc / (1 + 4 * w * w * tc * tc))
    assert -1.3 < sigma < -1.0 and 1.1 < rho < 1.4                  # s^-1: the size a 2.5 A proton pair in a slowly tumbling protein has
    for s2 in (1.0, 1.0 + 1e-9):                                    # an S2 that rounding took past 1 is clipped, not refused
        R = ctx.noesy_rates([r ** -6.0], [s2], 2, w, tc, 3e-11, 0.25, oracle.Q_ANGSTROM)
        assert abs(R[0, 1] - sigma) <= 64 * U53 * q * 7 * tc and R[0, 1] == R[1, 0]
        assert abs(R[0, 0] - (rho + 0.25)) <= 66 * U53 * (rho + 0.25) and R[0, 0] == R[1, 1]
    # the same pair in nanometres through the module
    m = dict(A6=np.array([0.25 ** -6.0]), S2=np.array([1.0]), index=np.array([4, 9]))
    R = noesy.rate_matrix(m, 600.0, tc, tau_e=3e-11, leak=0.25, unit='nm', ctx=ctx)
    assert abs(R[0, 1] - sigma) <= 1e-13 * abs(sigma) * 10 and abs(R[0, 0] - rho - 0.25) <= 1e-12


def test_rate_refusals_leave_the_context_usable(ctx):
    A6, S2, _ = oracle.synthetic(5)
    args = dict(A6=A6, S2=S2, P=5, tc=5e-9, te=5e-11, leak=0.5)
    good = ctx.noesy_rates(A6, S2, 5, W, 5e-9, 5e-11, 0.5, oracle.Q_ANGSTROM)

    def refused(pattern, **kw):
        a = dict(args, **kw)
        with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_noesy_rates_f64: .*' + pattern):
            ctx.noesy_rates(a['A6'], a['S2'], a['P'], W, a['tc'], a['te'], a['leak'], oracle.Q_ANGSTROM)
        assert ctx.noesy_rates(A6, S2, 5, W, 5e-9, 5e-11, 0.5, oracle.Q_ANGSTROM).tobytes() == good.tobytes()

    def changed(v, k, x):
        v = np.array(v)
        v[k] = x
        return v

    refused('a pair needs two', A6=np.zeros(0), S2=np.zeros(0), P=1)
    refused(r'A6\[3\] = nan', A6=changed(A6, 3, np.nan))
    refused(r'A6\[0\] = inf', A6=changed(A6, 0, np.inf))
    refused(r'A6\[9\] = 0 ', A6=changed(A6, 9, 0.0))
    refused(r'A6\[2\] = -', A6=changed(A6, 2, -1e-3))
    refused(r'S2\[4\] = 1.1', S2=changed(S2, 4, 1.1))
    refused(r'S2\[1\] = -0.001', S2=changed(S2, 1, -1e-3))
    refused(r'S2\[1\] = nan', S2=changed(S2, 1, np.nan))
    refused('tau_c = 0 ', tc=0.0)
    refused('tau_c = -', tc=-1e-9)
    refused('tau_e = 0 ', te=0.0)
    refused(r'tau_e\[7\] = -', te=changed(np.full(10, 5e-11), 7, -1e-11))
    refused('leak = -', leak=-0.1)
    refused(r'leak\[2\] = -', leak=changed(np.full(5, 0.5), 2, -0.5))


# ---- exponential ----
_expm_cache = {}


def expm_case(ctx, P, tc):
    """(R, A (len(TAUS), P, P)) once per case"""
    key = (P, tc)
    if key not in _expm_cache:
        R = oracle.synthetic_R(P, tc)
        A = noesy.intensities(R, TAUS, ctx=ctx)
        A.setflags(write=False)
        _expm_cache[key] = (R, A)
    return _expm_cache[key]


@pytest.mark.parametrize('tc', oracle.TAU_C)
@pytest.mark.parametrize('P', [2, 47, 65, 150])
def test_expm_against_both_references(ctx, P, tc):
    R, A = expm_case(ctx, P, tc)
    norm1 = np.abs(R).sum(axis=1).max()
    for tau in TAUS:
        assert hip.symm_expm_plan(norm1 * (1 + 1e-12), tau)[0] <= 8            # the range the bar was derived for
    assert A.shape == (len(TAUS), P, P)
    for k, tau in enumerate(TAUS):
        e1, e2 = np.max(np.abs(A[k] - oracle.expm_scipy(R, tau))), np.max(np.abs(A[k] - oracle.expm_eigh(R, tau)))
        print('P = %d tau_c = %g tau_m = %g: %.2e (expm) %.2e (eigh)' % (P, tc, tau, e1, e2))
        assert e1 <= 1e-12 and e2 <= 1e-12
        assert A[k].tobytes() == A[k].T.copy().tobytes()
        assert np.max(np.abs(A[k])) <= 1.0 + 1e-12
    assert np.array_equal(A[0], np.eye(P))                                      # tau = 0: the identity exactly


def test_expm_two_spin_closed_form(ctx):
    for tc in oracle.TAU_C:
        R, A = expm_case(ctx, 2, tc)
        rho, sigma = R[0, 0], R[0, 1]
        assert R[1, 1] == rho
        for k, tau in enumerate(TAUS):
            ep, em = np.exp(-(rho + sigma) * tau), np.exp(-(rho - sigma) * tau)
            assert abs(A[k, 0, 0] - 0.5 * (ep + em)) <= 1e-12 and abs(A[k, 0, 1] - 0.5 * (ep - em)) <= 1e-12


def test_expm_semigroup_and_alone_equals_list(ctx):
    for tc in oracle.TAU_C:
        R = oracle.synthetic_R(65, tc)
        A = noesy.intensities(R, [0.1, 0.2, 0.05], ctx=ctx)
        assert np.max(np.abs(A[1] - A[0] @ A[0])) <= 2e-12
        alone = noesy.intensities(R, [0.2], ctx=ctx)
        assert alone[0].tobytes() == A[1].tobytes()
        assert noesy.intensities(R, 0.05, ctx=ctx)[0].tobytes() == A[2].tobytes()
        assert expm_case(ctx, 65, tc)[1][2].tobytes() == A[1].tobytes()         # tau = 0.2 in yet another list


def test_sign_convention_at_short_mixing_time(ctx):
    """A = exp(-R tau) ~ 1 - R tau: at 1 ms every close pair has the sign of -sigma (negative sigma, slow tumbling: positive cross peaks)"""
    for tc in oracle.TAU_C:
        A6, S2, r = oracle.synthetic(65)
        R = oracle.synthetic_R(65, tc)
        A = noesy.intensities(R, [1e-3], ctx=ctx)[0]
        pr = oracle.pairs(65)
        close = r < 3.0
        assert close.sum() >= 10
        a, s = A[pr[close, 0], pr[close, 1]], R[pr[close, 0], pr[close, 1]]
        assert np.all(s != 0) and np.array_equal(np.sign(a), -np.sign(s))


def test_expm_refusals_leave_the_context_usable(ctx):
    import torch
    R = oracle.synthetic_R(5, 5e-9)
    good = noesy.intensities(R, [0.1], ctx=ctx)

    def still_good():
        assert noesy.intensities(R, [0.1], ctx=ctx).tobytes() == good.tobytes()

    def refused(pattern, M=R, taus=(0.1,)):
        with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_symm_expm_\w+: .*' + pattern):
            noesy.intensities(M, list(taus), ctx=ctx)
        still_good()

    bad = np.array(R)
    bad[1, 3] = bad[3, 1] = np.nan
    refused('R is not finite', M=bad)
    bad = np.array(R)
    bad[2, 2] = np.inf
    refused('R is not finite', M=bad)
    refused(r'mixing time 1 = -0.1', taus=(0.1, -0.1))
    refused(r'mixing time 0 = nan', taus=(np.nan,))
    refused(r'mixing time 0 = inf', taus=(np.inf,))
    refused('more than 40 squarings', M=R * 1e15)
    # results beyond the device's memory: 64 matrices of 32768 x 32768 float64 are 550 GB.  Refused before anything is allocated or
    # queued, by the check and by the call itself (which never touches the small arrays it is given here)
    with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_symm_expm_check: 64 x 32768 x 32768 x 8 bytes = 512.00 GiB of results .* do not fit the device'):
        ctx.symm_expm_check(32768, 64)
    still_good()
    R_d = to_dev(ctx, R)
    torch.cuda.synchronize()
    with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_symm_expm_f64_dev: 64 x 32768 x 32768 x 8 bytes = 512.00 GiB of results .* do not fit the device'):
        ctx.symm_expm_dev(R_d.data_ptr(), 32768, np.full(64, 0.1), R_d.data_ptr())
    still_good()
    with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_symm_expm_f64_dev: P=0'):
        ctx.symm_expm_dev(R_d.data_ptr(), 0, [0.1], R_d.data_ptr())
    with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_symm_expm_f64_dev: P=40000'):
        ctx.symm_expm_dev(R_d.data_ptr(), 40000, [0.1], R_d.data_ptr())
    with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_symm_mul_f64_dev: P=0'):
        ctx.symm_mul_dev(R_d.data_ptr(), R_d.data_ptr(), 0, R_d.data_ptr())
    with pytest.raises(SpinRelaxHipError, match=r'\(-3\): sr_symm_mul_f64_dev: alpha = nan'):
        ctx.symm_mul_dev(R_d.data_ptr(), R_d.data_ptr(), 5, R_d.data_ptr(), alpha=np.nan)
    still_good()
    assert np.array_equal(R_d.cpu().numpy(), R)


# ---- end to end ----
MIX = (0.05, 0.1, 0.2)


def numpy_chain(m, P):
    """the numpy chain from a map dict: coordinates in nm, 600 MHz, tau_c = 5 ns, tau_e = 50 ps, leak 0.5 / s"""
    return oracle.rate_matrix(m['A6'], m['S2'], P, W, 5e-9, oracle.TAU_E, oracle.LEAK, oracle.Q_NM)


def check_chain(out, m, P):
    ref, RHO, MAG = numpy_chain(m, P)
    R = out['R']
    off = ~np.eye(P, dtype=bool)
    assert np.all(np.abs(R - ref)[off] <= 64 * U53 * MAG[off])
    assert np.all(np.abs(np.diagonal(R) - np.diagonal(ref)) <= P * U53 * RHO.sum(axis=1) + 64 * U53 * np.diagonal(ref))
    norm1 = np.abs(ref).sum(axis=1).max()
    for k, tau in enumerate(out['mixing_times']):
        assert hip.symm_expm_plan(norm1 * (1 + 1e-12), tau)[0] <= 8
        assert np.max(np.abs(out['A'][k] - oracle.expm_scipy(ref, tau))) <= 1e-12
        assert np.max(np.abs(out['A'][k] - oracle.expm_eigh(ref, tau))) <= 1e-12
    pr = oracle.pairs(P)
    assert np.array_equal(out['sigma'], R[pr[:, 0], pr[:, 1]]) and np.array_equal(out['rho'], np.diagonal(R))
    assert np.array_equal(out['pairs'], pr)


def test_map_to_noesy_end_to_end(ctx):
    P, F = 24, 2000
    _, xyz, quat = make_body(P, F)
    m = noe.dipolar_map(xyz, np.arange(P), quat=quat, blocks=([0, 500, 1000, 1500], [500] * 4), mode=0, ctx=ctx)
    out = noesy.noesy(m, MIX, 600.0, 5e-9, tau_e=oracle.TAU_E, leak=oracle.LEAK, unit='nm', ctx=ctx)
    assert out['A'].shape == (3, P, P) and np.array_equal(out['mixing_times'], MIX)
    check_chain(out, m, P)
    assert np.abs(out['A'][2][~np.eye(P, dtype=bool)]).max() > 1e-3              # there are cross peaks to speak of
    # the two steps apart give the same bits as the chain that leaves R on the device
    R = noesy.rate_matrix(m, 600.0, 5e-9, tau_e=oracle.TAU_E, leak=oracle.LEAK, unit='nm', ctx=ctx)
    assert R.tobytes() == out['R'].tobytes()
    assert noesy.intensities(R, MIX, ctx=ctx).tobytes() == out['A'].tobytes()


def test_cli_noesy_outputs_and_nothing_else_changes(tmp_path, ctx):
    P, F = 24, 2000
    body, xyz, _ = make_body(P, F)
    names = ['H%d' % a for a in range(P)]
    ref32 = body.astype(np.float32)
    fn = str(tmp_path / 'traj.npz')
    gfn = str(tmp_path / 'groups.txt')
    with open(gfn, 'w') as fp:
        fp.write('# a methyl and two singles\n0 1 2\n5\n7 # the last\n')
    np.savez(fn, xyz=xyz, indexX=np.array([0, 2, 3]), indexH=np.array([1, 4, 5]), ref_xyz=ref32, fit_indices=np.arange(P), indexP=np.arange(P),
             namesP=np.array(names), dt=np.float32(1.0))
    script = os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')
    common = ['-s', 'none.pdb', '-f', fn, '--tau', '500', '--S2', '--noeMap', '--binary']
    extra = ['--noesy', '--noesyMix', ' '.join('%g' % t for t in MIX), '--noesyField', '600', '--noesyTauC', '5e-9', '--noesyTauE', '5e-11',
             '--noesyLeak', '0.5', '--noesyUnit', 'nm', '--noesyGroups', gfn]
    dirs = []
    for name, more in (('map', []), ('noesy', extra)):
        d = tmp_path / name
        d.mkdir()
        p = subprocess.run([sys.executable, script] + common + ['-o', str(d / 'o')] + more, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=300)
        assert p.returncode == 0, p.stdout.decode()[-3000:]
        dirs.append(d)
    before, after = (sorted(os.listdir(str(d))) for d in dirs)
    assert sorted(before + ['o_noesy.dat', 'o_noesy.npz', 'o_noesyGroups.dat']) == after
    for f in before:                                # every earlier output is what it was: text byte for byte, the arrays of an .npz bit for bit
        a, b = str(dirs[0] / f), str(dirs[1] / f)
        if f.endswith('.npz'):
            za, zb = np.load(a, allow_pickle=True), np.load(b, allow_pickle=True)
            assert sorted(za.files) == sorted(zb.files)
            for k in za.files:
                assert za[k].tobytes() == zb[k].tobytes() and za[k].dtype == zb[k].dtype, (f, k)
        else:
            assert open(a, 'rb').read() == open(b, 'rb').read(), f
    # the table against the module on the map the script saved
    z = np.load(str(dirs[1] / 'o_noeMap.npz'))
    m = dict(A6=z['A6'], S2=z['S2'], index=z['index'])
    out = noesy.noesy(m, MIX, 600.0, 5e-9, tau_e=5e-11, leak=0.5, unit='nm', ctx=ctx)
    check_chain(out, m, P)
    zn = np.load(str(dirs[1] / 'o_noesy.npz'))
    assert zn['A'].tobytes() == out['A'].tobytes() and zn['R'].tobytes() == out['R'].tobytes()
    tab = noesy.read_noesy(str(dirs[1] / 'o_noesy.dat'))
    ii, jj = np.triu_indices(P)
    assert np.array_equal(tab['i'], ii) and np.array_equal(tab['j'], jj) and tab['name_j'] == [names[j] for j in jj]
    assert np.array_equal(tab['mixing_times'], MIX)
    want = out['A'][:, ii, jj].T
    assert np.all(np.abs(tab['A'] - want) <= 5e-8 * np.abs(want)) and np.all(np.abs(tab['sigma'] - out['R'][ii, jj]) <= 5e-8 * np.abs(out['R'][ii, jj]))
    grp = noesy.read_noesy(str(dirs[1] / 'o_noesyGroups.dat'))
    G = noesy.sum_groups(out['A'], [[0, 1, 2], [5], [7]])
    gi, gj = np.triu_indices(3)
    assert grp['name_i'] == ['G%d' % g for g in gi] and np.all(np.abs(grp['A'] - G[:, gi, gj].T) <= 5e-8 * np.abs(G[:, gi, gj].T))
