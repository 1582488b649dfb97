"""
CPU tests of the host side of NOESY under anisotropic tumbling: noe.mode_amplitudes / mode_plateau / mode_tau_e / finalize_modes, the
D= keyword of noesy.rate_matrix and noesy.noesy, and the --noesyD flag of scripts/calculate-Ct-from-traj.py.  No GPU: everything that
would need one is refused before a context is asked for, which is what these tests check.

rates_modes_numpy below restates the rate definition in numpy; tests/test_gpu_noe_modes.py holds k_noesy_rates_modes to it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import noesy_oracle as orc
from conftest import ROOT
from spinrelax_amd import _hostmath as hm
from spinrelax_amd import noe, noesy

TENSORS = [np.array(D) * 1e7 for D in ((1.0, 1.0, 1.0), (1.0, 1.0, 1.6), (1.6, 1.0, 1.0), (0.8, 1.0, 1.5))]   # sphere, prolate, oblate, rhombic


def unit_vectors(n, seed):
    u = np.random.default_rng(seed).standard_normal((n, 3))
    return u / np.linalg.norm(u, axis=1)[:, None]


def H_of(u, v, w=1.0, symmetric=True):
    """the six mode sums of one term: unit vectors u, v (n, 3), weight w; symmetric=False: H2 = qz(u) dl(v) alone"""
    qu, qv = u[:, 2] ** 2 - 1.0 / 3.0, v[:, 2] ** 2 - 1.0 / 3.0
    du, dv = u[:, 0] ** 2 - u[:, 1] ** 2, v[:, 0] ** 2 - v[:, 1] ** 2
    h2 = 0.5 * (qu * dv + du * qv) if symmetric else qu * dv
    return w * np.stack((qu * qv, du * dv, h2, u[:, 1] * u[:, 2] * v[:, 1] * v[:, 2], u[:, 0] * u[:, 2] * v[:, 0] * v[:, 2],
                         u[:, 0] * u[:, 1] * v[:, 0] * v[:, 1]), axis=-1)


def g(x, y):
    return x / (x * x + y * y)


def rates_modes_numpy(a, c, E, P, w, te, leak, q):
    """R (P, P), rho per pair as a symmetric matrix with zero diagonal, and the five-term magnitude sum q (|J(0)| + 6 |J(2w)|) that
    bounds sigma's rounding: a, c (npairs, 5), E (5), te a scalar, (npairs) or (npairs, 5)"""
    a, c, E = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64), np.asarray(E, dtype=np.float64)
    te = np.broadcast_to(np.asarray(te, dtype=np.float64).reshape((-1, 1) if np.ndim(te) == 1 else np.shape(te)), a.shape)
    d = np.maximum(a - c, 0.0)
    Ef = E[None] + 1.0 / te

    def J(om):
        return (c * g(E[None], om) + d * g(Ef, om)).sum(axis=1)
    J0, J1, J2 = J(0.0), J(w), J(2.0 * w)
    pr = orc.pairs(P)

    def full(v):
        M = np.zeros((P, P))
        M[pr[:, 0], pr[:, 1]] = v
        M[pr[:, 1], pr[:, 0]] = v
        return M
    R, RHO, MAG = full(q * (6.0 * J2 - J0)), full(q * (J0 + 3.0 * J1 + 6.0 * J2)), full(q * (J0 + 6.0 * J2))
    R[np.arange(P), np.arange(P)] = RHO.sum(axis=1) + leak
    return R, RHO, MAG


# ---- mode algebra ----
@pytest.mark.parametrize('D', TENSORS)
def test_amplitudes_of_one_vector_are_A_coefficients_ellipsoid(D):
    u = unit_vectors(200, 1)
    got = noe.mode_amplitudes(H_of(u, u), D)
    want = hm.A_coefficients_ellipsoid(u, D)
    assert got.shape == (200, 5) and np.max(np.abs(got - want)) <= 1e-14
    assert np.max(np.abs(got.sum(axis=1) - 1.0)) <= 1e-14


@pytest.mark.parametrize('D', TENSORS)
def test_mode_sum_is_P2_for_two_vectors(D):
    u, v = unit_vectors(200, 2), unit_vectors(200, 3)
    w = np.random.default_rng(4).uniform(0.5, 2.0, 200)
    Q = u[:, :, None] * u[:, None, :] - np.eye(3) / 3.0
    Qp = v[:, :, None] * v[:, None, :] - np.eye(3) / 3.0
    want = w * 1.5 * np.einsum('nab,nab->n', Q, Qp)
    got = noe.mode_amplitudes(H_of(u, v, w[:, None]), D).sum(axis=1)
    assert np.max(np.abs(got - want)) <= 1e-14
    assert np.max(np.abs(want - w * (1.5 * (u * v).sum(axis=1) ** 2 - 0.5))) <= 1e-14          # and 1.5 Q : Q' is P2(u . v)


def test_modes_are_symmetric_in_the_two_vectors_and_H2_must_be_symmetrised():
    """g_m(u, v) = g_m(v, u) (a correlation function of a stationary process is even); with H2 = qz(u) dl(v) alone the modes 3 and 4 of
    a rhombic tensor differ from the symmetrised form and lose that symmetry (their sum, P2, does not see it)"""
    D = TENSORS[3]
    u, v = np.array([[0.0, 0.6, 0.8]]), np.array([[0.6, 0.0, 0.8]])
    a, b = noe.mode_amplitudes(H_of(u, v), D), noe.mode_amplitudes(H_of(v, u), D)
    assert np.max(np.abs(a - b)) <= 1e-15
    raw, raw_T = noe.mode_amplitudes(H_of(u, v, symmetric=False), D), noe.mode_amplitudes(H_of(v, u, symmetric=False), D)
    assert abs(raw[0, 3] - a[0, 3]) > 1e-3 and abs(raw[0, 3] - raw_T[0, 3]) > 1e-3
    assert abs(raw.sum() - a.sum()) <= 1e-15


def test_amplitudes_are_linear_and_broadcast():
    rng = np.random.default_rng(5)
    H = rng.standard_normal((3, 4, 6))
    D = TENSORS[3]
    assert noe.mode_amplitudes(H, D).shape == (3, 4, 5)
    assert np.max(np.abs(noe.mode_amplitudes(H[0] + 2 * H[1], D) - noe.mode_amplitudes(H[0], D) - 2 * noe.mode_amplitudes(H[1], D))) <= 1e-14
    with pytest.raises(ValueError, match=r'\(\.\.\., 6\)'):
        noe.mode_amplitudes(H[..., :5], D)
    for bad in ((1.0, 1.0), (1.0, 1.0, 0.0), (1.0, np.nan, 1.0), (-1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match='D must be'):
            noe.mode_amplitudes(H, bad)


# ---- plateau ----
def rot(q):
    return noe.frame_matrix(q)


Q_F = np.array([0.5, -0.1, 0.7, 0.3]) / np.linalg.norm([0.5, -0.1, 0.7, 0.3])


@pytest.mark.parametrize('D', TENSORS)
def test_plateau_of_a_rigid_pair(D):
    """T = u u^T r^-3: c = r^-6 A(u); with a frame quaternion c = r^-6 A(F u), and rotating T by hand is the same"""
    u = unit_vectors(50, 6)
    r = np.random.default_rng(7).uniform(0.2, 0.6, 50)
    T = u[:, :, None] * u[:, None, :] * (r ** -3)[:, None, None]
    got = noe.mode_plateau(T, D)
    want = (r ** -6)[:, None] * hm.A_coefficients_ellipsoid(u, D)
    assert np.max(np.abs(got / want.sum(axis=1)[:, None] - want / want.sum(axis=1)[:, None])) <= 1e-13
    F = rot(Q_F)
    got_F = noe.mode_plateau(T, D, Q_F)
    want_F = (r ** -6)[:, None] * hm.A_coefficients_ellipsoid(u @ F.T, D)
    assert np.max(np.abs(got_F - want_F) / want.sum(axis=1)[:, None]) <= 1e-13
    by_hand = noe.mode_plateau(np.einsum('ab,nbc,dc->nad', F, T, F), D)
    assert np.max(np.abs(got_F - by_hand) / want.sum(axis=1)[:, None]) <= 1e-13
    # the sum over the modes is the map's S2 A6 = 1.5 (T : T - (tr T)^2 / 3), whatever the frame
    s2a6 = 1.5 * (np.einsum('nab,nab->n', T, T) - np.trace(T, axis1=1, axis2=2) ** 2 / 3.0)
    assert np.max(np.abs(got_F.sum(axis=1) / s2a6 - 1)) <= 1e-13


def test_frame_matrix_is_vecRots_convention():
    """R(q) v is the vector part of q (0, v) q*, what --vecRot applies (quaternions.rotate_vector)"""
    from spinrelax_amd import quaternions as qops
    v = np.array([0.3, -1.2, 0.5])
    assert np.max(np.abs(rot(Q_F) @ v - qops.rotate_vector(v, Q_F))) <= 1e-15
    assert np.array_equal(rot(None), np.eye(3))
    for bad in ([1.0, 0.0, 0.0], [1.0, 0.1, 0.0, 0.0], [np.nan, 0.0, 0.0, 1.0]):
        with pytest.raises(ValueError, match='unit quaternion'):
            noe.frame_matrix(bad)


# ---- a hand-made map: finalize_modes, mode_tau_e, the inputs of the rate kernel ----
def hand_made_map(P=4, K=6, tau=5.0, seed=8):
    """a map dict as dipolar_map(..., modes=True) makes it, of pairs whose unit vector jumps between two directions: the mode
    functions are a_m at lag 0 and decay as exp(-k / tau) to c_m, exactly"""
    rng = np.random.default_rng(seed)
    n = noe.n_pairs(P)
    u1, u2 = unit_vectors(n, seed + 1), unit_vectors(n, seed + 2)
    r = rng.uniform(0.2, 0.5, n)
    w = r ** -6
    lags = np.arange(K) * 2
    # two equally populated states: <f(u(0)) f(u(k))> = mean-of-products e^{-k / tau} + product-of-means (1 - e^{-k / tau})
    same = 0.5 * (H_of(u1, u1) + H_of(u2, u2))
    cross = 0.25 * (H_of(u1, u1) + H_of(u2, u2) + H_of(u1, u2) + H_of(u2, u1))
    decay = np.exp(-lags / tau)[:, None, None]
    H = w[None, :, None] * (decay * same[None] + (1 - decay) * cross[None])
    T = 0.5 * (u1[:, :, None] * u1[:, None, :] + u2[:, :, None] * u2[:, None, :]) * (r ** -3)[:, None, None]
    return dict(H=H, T=T, lags=lags, dt=1.0, index=np.arange(P), frame=np.array([1.0, 0.0, 0.0, 0.0]), A6=w,
                S2=1.5 * (np.einsum('nab,nab->n', T, T) - np.trace(T, axis1=1, axis2=2) ** 2 / 3.0) / w)


def test_plateau_is_the_long_time_limit_and_tau_e_per_mode():
    m = hand_made_map(K=40, tau=5.0)
    D = TENSORS[3]
    c = noe.mode_plateau(m['T'], D)
    far = noe.mode_amplitudes(m['H'][-1], D)                     # lag 78: e^{-15.6}
    assert np.max(np.abs(far - c) / m['A6'][:, None]) <= 1e-6
    a = noe.mode_amplitudes(m['H'][0], D)
    assert np.all(a - c >= -1e-12 * m['A6'][:, None]) and np.max(np.abs(a.sum(axis=1) / m['A6'] - 1)) <= 1e-13
    assert np.max(np.abs(c.sum(axis=1) / (m['S2'] * m['A6']) - 1)) <= 1e-12
    te = noe.mode_tau_e(m, D)
    assert te.shape == (noe.n_pairs(4), 5)
    # every mode decays as exp(-k / 5): the trapezoid rule at spacing 2 gives 2 (1/2 + sum_{k >= 1} e^{-2k/5}) = coth(1/5) = 5.0663
    live = (a - c) > 1e-9 * m['A6'][:, None]
    assert live.sum() > 0.8 * live.size
    assert np.max(np.abs(te[live] - 1.0 / np.tanh(0.2))) <= 1e-3
    # in seconds, floored, as the rate matrix takes it
    ms = dict(m, dt=1e-12)
    fl = noesy.mode_tau_e(ms, D)
    assert np.all(fl >= noesy.TAU_E_FLOOR) and np.max(np.abs(fl[live] / 1e-12 - 1.0 / np.tanh(0.2))) <= 1e-3
    # a rigid map: a = c, every mode gets the floor
    u = unit_vectors(noe.n_pairs(4), 3)
    rigid = dict(m, H=np.broadcast_to(H_of(u, u)[None], m['H'].shape), T=u[:, :, None] * u[:, None, :], A6=np.ones(u.shape[0]))
    assert np.all(noesy.mode_tau_e(dict(rigid, dt=1e-12), D) == noesy.TAU_E_FLOOR)


def test_finalize_modes_averages_over_the_origins_of_ragged_blocks():
    rng = np.random.default_rng(9)
    bl, lags = [37, 20, 40], [0, 1, 5, 19]
    Hb = rng.standard_normal((3, 4, 6, 6))
    out = noe.finalize_modes(Hb, bl, lags, Q_F)
    for q, k in enumerate(lags):
        assert np.max(np.abs(out['H'][q] - Hb[:, q].sum(axis=0) / sum(n - k for n in bl))) <= 1e-15
    assert out['H_blocks'] is not None and np.array_equal(out['frame'], Q_F)
    assert np.array_equal(noe.finalize_modes(Hb, bl, lags)['frame'], [1.0, 0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match='every lag must leave a term'):
        noe.finalize_modes(Hb, bl, [0, 1, 5, 20])
    with pytest.raises(ValueError, match=r'\(blocks, lags, pairs, 6\)'):
        noe.finalize_modes(Hb[..., :5], bl, lags)


def test_mode_inputs_take_the_rounding_out():
    m = hand_made_map()
    D = TENSORS[1]
    m['H'] = m['H'].copy()
    m['H'][0, 0] *= 1 - 1e-7                                     # a below c by rounding for a rigid-like pair
    a, c, E = noesy.mode_inputs(m, D)
    assert np.all(a >= 0) and np.all(c >= 0) and np.all(c <= a) and np.array_equal(E, hm.D_coefficients_ellipsoid(D))


# ---- rates: the definition, restated ----
@pytest.mark.parametrize('P', (2, 47))
@pytest.mark.parametrize('tc', orc.TAU_C)
def test_isotropic_limit_of_the_rate_definition(P, tc):
    """a_m, c_m any split of A6 and S2 A6 over the five modes and E_m = 1 / tc for all: the oracle's isotropic matrix to 1e-13 of its
    magnitude arrays"""
    A6, S2, _ = orc.synthetic(P)
    w = orc.omega_H(orc.FIELD)
    split = np.random.default_rng(P).dirichlet(np.ones(5), A6.size)
    a, c = A6[:, None] * split, (S2 * A6)[:, None] * split
    R, RHO, MAG = rates_modes_numpy(a, c, np.full(5, 1.0 / tc), P, w, orc.TAU_E, orc.LEAK, orc.Q_ANGSTROM)
    R0, RHO0, MAG0 = orc.rate_matrix(A6, S2, P, w, tc, orc.TAU_E, orc.LEAK, orc.Q_ANGSTROM)
    off = ~np.eye(P, dtype=bool)
    assert np.max(np.abs(R - R0)[off] / MAG0[off]) <= 1e-13
    assert np.max(np.abs(RHO - RHO0)[off] / RHO0[off]) <= 1e-13 and np.max(np.abs(MAG - MAG0)[off] / MAG0[off]) <= 1e-13
    assert np.max(np.abs(np.diagonal(R) - np.diagonal(R0)) / np.diagonal(R0)) <= 1e-13
    # and with the sphere's tensor through the package's own rates
    E = hm.D_coefficients_ellipsoid(np.full(3, 1.0 / (6.0 * tc)))
    assert np.max(np.abs(E * tc - 1)) <= 1e-15


def test_rate_definition_of_a_rigid_pair_is_J_combine_ellipsoid():
    """one rigid pair along u, tensor rhombic: J of the definition is r^-6 _hostmath.J_combine_ellipsoid_exp_decayN(w, u, D, 1, [], [])"""
    D = TENSORS[3]
    u = unit_vectors(1, 11)
    r, w, q = 0.25, orc.omega_H(600.0), orc.Q_NM
    a = r ** -6 * hm.A_coefficients_ellipsoid(u, D)
    R, RHO, _ = rates_modes_numpy(a, a, hm.D_coefficients_ellipsoid(D), 2, w, 1e-10, 0.0, q)
    Jw = hm.J_combine_ellipsoid_exp_decayN([0.0, w, 2 * w], u, D, 1.0, [], [])[0]
    assert abs(R[0, 1] / (q * r ** -6 * (6 * Jw[2] - Jw[0])) - 1) <= 1e-13
    assert abs(RHO[0, 1] / (q * r ** -6 * (Jw[0] + 3 * Jw[1] + 6 * Jw[2])) - 1) <= 1e-13


# ---- every ValueError path, no context created ----
def no_context(monkeypatch):
    from spinrelax_amd import hip

    def boom(*a, **k):
        raise AssertionError('a context was asked for')
    monkeypatch.setattr(hip, 'default_context', boom)
    monkeypatch.setattr(hip, 'Context', boom)


def test_map_refusals_before_a_context(monkeypatch):
    no_context(monkeypatch)
    xyz = np.zeros((30, 4, 3), dtype=np.float32)
    idx = np.arange(4)
    for fn, args in ((noe.dipolar_map, (xyz, idx)), (noe.dipolar_map_superposed, (xyz, xyz[0], idx, idx))):
        with pytest.raises(ValueError, match='lags that start at 0'):
            fn(*args, modes=True, lags=[1, 2, 4])
        with pytest.raises(ValueError, match='unit quaternion'):
            fn(*args, modes=True, frame=[1.0, 1.0, 0.0, 0.0])
        with pytest.raises(ValueError, match='unit quaternion'):
            fn(*args, modes=True, frame=[1.0, 0.0, 0.0])
        with pytest.raises(ValueError, match='unit quaternion'):
            fn(*args, modes=True, frame=[np.inf, 0.0, 0.0, 0.0])
        with pytest.raises(ValueError, match='frame belongs to modes=True'):
            fn(*args, frame=[1.0, 0.0, 0.0, 0.0])
        with pytest.raises(ValueError, match='lags must be'):
            fn(*args, modes=True, lags=[0.5, 1.0])


def test_rate_refusals_before_a_context(monkeypatch):
    no_context(monkeypatch)
    m = hand_made_map()
    plain = {k: v for k, v in m.items() if k != 'H'}
    D = TENSORS[3]
    for fn, args in ((noesy.rate_matrix, (600.0,)), (noesy.noesy, ([0.1], 600.0))):
        with pytest.raises(ValueError, match='modes=True'):
            fn(plain, *args, D=D)
        with pytest.raises(ValueError, match='tau_c must be None'):
            fn(m, *args, 5e-9, D=D)
        with pytest.raises(ValueError, match='tau_c, or the diffusion tensor'):
            fn(m, *args)
        for bad in ((1e7, 1e7), (1e7, 0.0, 1e7), (1e7, np.nan, 1e7)):
            with pytest.raises(ValueError, match='D must be'):
                fn(m, *args, D=bad)
        with pytest.raises(ValueError, match="'map' or 'modes'"):
            fn(m, *args, D=D, tau_e='auto')
        with pytest.raises(ValueError, match="or 'map'$"):
            fn(m, *args, 5e-9, tau_e='modes')                     # 'modes' belongs to D
        with pytest.raises(ValueError, match='holds no tau_e'):
            fn(m, *args, D=D, tau_e='map')
        with pytest.raises(ValueError, match='lags beyond 0'):
            fn(dict(m, H=m['H'][:1], lags=m['lags'][:1]), *args, D=D, tau_e='modes')
    with pytest.raises(ValueError, match='holds no H'):
        noe.mode_tau_e(plain, D)


def test_cli_noesyD_refusals_without_gpu(tmp_path):
    """--noesyD against the flags it does not fit: the script's '= = = ERROR:' message and exit status 1 before any GPU work: the input
    file does not even exist"""
    script = os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')
    base = [sys.executable, script, '-s', 'none.pdb', '-f', str(tmp_path / 'missing.npz'), '-o', str(tmp_path / 'o')]
    full = ['--noeMap', '--noesy', '--noesyMix', '0.05 0.1', '--noesyField', '600']
    cases = [(['--noeMap', '--noesyD', '1e7 1.3'], '--noesyD belongs to --noesy'),
             (full + ['--noesyD', '1e7 1.3', '--noesyTauC', '5e-9'], '--noesyD and --noesyTauC both describe the tumbling'),
             (full, '--noesy needs --noesyTauC'),
             (full + ['--noesyD', '1e7'], '--noesyD must be'),
             (full + ['--noesyD', '1e7 1.3 0.2 4'], '--noesyD must be'),
             (full + ['--noesyD', '1e7 x'], '--noesyD must be'),
             (full + ['--noesyD', '-1e7 1.3'], '--noesyD must be'),
             (full + ['--noesyD', '1e7 1.3 12.0'], '--noesyD must be'),                      # Dx = Dperp - h < 0
             (full + ['--noesyD', '1e7 1.3', '--vecRot', '1 0 0'], '--noesyD takes --vecRot'),
             (full + ['--noesyD', '1e7 1.3', '--vecRot', '1 1 0 0'], '--noesyD takes --vecRot'),
             (full + ['--noesyD', '1e7 1.3', '--noesyTauEMap'], '--noesyTauEMap takes tau_e from the lagged map')]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for extra, msg in cases:
        p = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
        err = p.stderr.decode()
        assert p.returncode == 1 and ('= = = ERROR: ' in err) and msg in err, (extra, p.returncode, err[-500:])
        assert not os.listdir(str(tmp_path))


def test_signatures_present():
    from spinrelax_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        from spinrelax_amd import build
        build.build(verbose=False)
    lib = _lib.load()
    for name in ('sr_noe_modes_f32_dev', 'sr_noe_modes_f32', 'sr_noe_modes_check', 'sr_noesy_rates_modes_f64_dev', 'sr_noesy_rates_modes_f64'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
