"""
CPU tests of the host side of the mode-resolved bond-vector C(t): spinrelax_amd/modes.py (amplitudes, pl_transform, J, relaxation)
and the --modeCt / --modeD / --modeField flag checks of scripts/calculate-Ct-from-traj.py.  No GPU: the six mode sums come from
oracle_modes below, the definition in float64 numpy, which tests/test_gpu_ct_modes.py also holds k_ct_modes to.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import integrate

import ellipsoid_oracle as eo
from conftest import ROOT
from spinrelax_amd import _hostmath as hm
from spinrelax_amd import modes, noe

U53 = 2.0 ** -53
TENSORS = [np.array(D) * 2.0e-5 for D in ((1.0, 1.0, 1.8), (1.7, 1.0, 1.0), (0.8, 1.0, 1.5))]      # prolate, oblate, rhombic; 1/ps
FRAME = np.array([0.4, -0.5, 0.3, 0.7]) / np.linalg.norm([0.4, -0.5, 0.3, 0.7])


def signals(u):
    """unit vectors u (..., 3) float64 -> the five signals (..., 5)"""
    x, y, z = u[..., 0], u[..., 1], u[..., 2]
    return np.stack((z * z - 1.0 / 3.0, x * x - y * y, y * z, x * z, x * y), axis=-1)


def sums_of_signals(s4):
    """s4 (R, F, V, 5) float64 -> per chunk S (R, L + 1, V, 6) = the six plain sums / (F - k), and sum|terms| / (F - k) alike"""
    R, F = s4.shape[:2]
    L = F // 2
    S = np.empty((R, L + 1, s4.shape[2], 6))
    A = np.empty_like(S)
    for k in range(L + 1):
        a, b = s4[:, :F - k], s4[:, k:]
        t = [a[..., 0] * b[..., 0], a[..., 1] * b[..., 1], None, a[..., 2] * b[..., 2], a[..., 3] * b[..., 3], a[..., 4] * b[..., 4]]
        t01, t10 = a[..., 0] * b[..., 1], a[..., 1] * b[..., 0]
        for c in range(6):
            if c == 2:
                S[:, k, :, c] = 0.5 * (t01.sum(axis=1) + t10.sum(axis=1)) / (F - k)
                A[:, k, :, c] = 0.5 * (np.abs(t01).sum(axis=1) + np.abs(t10).sum(axis=1)) / (F - k)
            else:
                S[:, k, :, c] = t[c].sum(axis=1) / (F - k)
                A[:, k, :, c] = np.abs(t[c]).sum(axis=1) / (F - k)
    return S, A


def oracle_modes(s4):
    """the library's results from the signals s4 (R, F, V, 5): dict(H, dH, smean, frame, lags) and absH / absH_max = mean / largest
    over the chunks of sum|terms| / (F - k), what the rounding bars scale with"""
    s4 = np.asarray(s4, dtype=np.float64)
    R, F = s4.shape[:2]
    S, A = sums_of_signals(s4)
    with np.errstate(divide='ignore', invalid='ignore'):
        dH = np.std(S, axis=0) / (np.sqrt(R) - 1.0)
    return dict(H=S.mean(axis=0), dH=dH, smean=s4.mean(axis=(0, 1)), frame=np.array([1.0, 0, 0, 0]), lags=np.arange(F // 2 + 1),
                absH=A.mean(axis=0), absH_max=A.max(axis=0))


def mobile_vectors(N, nV, seed):
    """unit vectors (N, nV, 3) float64: a random walk on the sphere plus jumps between two sites 70 degrees apart"""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((nV, 3))
    base /= np.linalg.norm(base, axis=1)[:, None]
    perp = np.cross(base, rng.standard_normal((nV, 3)))
    perp /= np.linalg.norm(perp, axis=1)[:, None]
    site = np.zeros(nV, dtype=int)
    u = base.copy()
    out = np.empty((N, nV, 3))
    ang = np.radians(35.0)
    for t in range(N):
        flip = rng.random(nV) < 0.02
        site = np.where(flip, 1 - site, site)
        centre = np.cos(ang) * base + np.where(site[:, None] == 1, 1.0, -1.0) * np.sin(ang) * perp
        u = u + 0.08 * rng.standard_normal((nV, 3)) + 0.1 * (centre - u)
        u /= np.linalg.norm(u, axis=1)[:, None]
        out[t] = u
    return out


# ---- pl_transform -------------------------------------------------------------------------------------------------------------
def quad_transform(f, h, z):
    n = len(f)
    t = np.arange(n) * h
    re = integrate.quad(lambda x: np.interp(x, t, f) * np.exp(-z.real * x) * np.cos(z.imag * x), 0.0, t[-1], points=t[1:-1], limit=50 * n,
                        epsabs=0.0, epsrel=2e-14)
    im = integrate.quad(lambda x: -np.interp(x, t, f) * np.exp(-z.real * x) * np.sin(z.imag * x), 0.0, t[-1], points=t[1:-1], limit=50 * n,
                        epsabs=0.0, epsrel=2e-14)
    return re[0] + 1j * im[0], re[1] + im[1]


@pytest.mark.parametrize('zh', [4e-3, 0.8, 2.5, 0.4999, 0.5001])
def test_pl_transform_against_quad(zh):
    """|z h| = 4e-3 (the series), 0.8 and 2.5 (the closed form) and either side of the switch at 0.5; bar: quad's own error estimate
    plus 64 roundings of the weighted sum"""
    rng = np.random.default_rng(5)
    f = np.exp(-0.3 * np.arange(14)) + 0.1 * rng.standard_normal(14)
    h = 0.37
    z = zh / h * np.exp(1j * 1.1)
    got = modes.pl_transform(f, h, z)
    want, err = quad_transform(f, h, z)
    bar = err + 64 * U53 * h * np.abs(f).sum()
    print('zh %.4g: |diff| %.2e bar %.2e rel %.2e' % (zh, abs(got - want), bar, abs(got - want) / abs(want)))
    assert abs(got - want) <= bar
    assert abs(got - want) <= 1e-13 * abs(want)


def test_pl_transform_shapes_and_one_sample():
    f = np.random.default_rng(6).standard_normal((9, 3))
    z = np.array([0.2 + 1j, 0.1 - 2j])
    got = modes.pl_transform(f[:, :, None], 0.5, z[None, :])
    assert got.shape == (3, 2)
    for i in range(3):
        for j in range(2):
            assert abs(got[i, j] - modes.pl_transform(f[:, i], 0.5, z[j])) <= 1e-15 * np.abs(f).sum()
    assert np.all(modes.pl_transform(f[:1, 0], 0.5, z) == 0)
    # real z = 0: the trapezoid rule
    assert abs(modes.pl_transform(f[:, 0], 0.5, 0.0) - 0.5 * (f[:-1, 0] + f[1:, 0]).sum() * 0.5) <= 1e-14 * np.abs(f).sum()


# ---- the six sums ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mobile():
    R, F, V = 3, 60, 4
    u = mobile_vectors(R * F, V, seed=12)
    Fm = noe.frame_matrix(FRAME)
    ur = u @ Fm.T
    res = oracle_modes(signals(ur).reshape(R, F, V, 5))
    res['frame'] = FRAME
    return u.reshape(R, F, V, 3), ur.reshape(R, F, V, 3), res


def test_lag0_amplitudes_are_the_frame_mean_of_A(mobile):
    _, ur, res = mobile
    for D in TENSORS:
        a, c, E = modes.amplitudes(res, D)
        want = hm.A_coefficients_ellipsoid(ur, D).mean(axis=(0, 1))
        assert np.max(np.abs(a[0] - want)) <= 32 * U53
        assert np.max(np.abs(E - hm.D_coefficients_ellipsoid(D))) == 0
        assert c.shape == (ur.shape[2], 5) and np.all(c.sum(axis=1) <= a[0].sum(axis=1) + 1e-15)


def test_six_sum_identity_against_P2(mobile):
    u, _, res = mobile
    R, F = u.shape[:2]
    H = res['H']
    C = 2.25 * H[..., 0] + 0.75 * H[..., 1] + 3.0 * (H[..., 3] + H[..., 4] + H[..., 5])
    for k in range(F // 2 + 1):
        d = np.einsum('rtvc,rtvc->rtv', u[:, :F - k], u[:, k:])
        want = (1.5 * d * d - 0.5).mean(axis=1).mean(axis=0)
        assert np.max(np.abs(C[k] - want)) <= 64 * U53
    # and the sum of the five mode functions, whatever the tensor
    a, c, _ = modes.amplitudes(res, TENSORS[2])
    assert np.max(np.abs(a.sum(axis=-1) - C)) <= 64 * U53


# ---- J and the rates ------------------------------------------------------------------------------------------------------------
def constants(field_MHz):
    from spinrelax_amd.spectral_densities import relaxationModel
    R = relaxationModel('NH', 2.0 * np.pi * field_MHz * 1e6 / 267.513e6)
    R.set_time_unit('ps')
    return R, R.get_f_DD(), R.get_f_CSA(), R.time_fact, R.gH.gamma / R.gX.gamma


@pytest.mark.parametrize('stop', ['crossing', 'end'])
def test_rigid_vectors_equal_the_closed_form(stop):
    """rigid vectors in a non-trivial frame: a_m(k) = c_m = A_m(u), so J = sum_m A_m g(E_m, w): ellipsoid_oracle.J_closed with S2 = 1,
    and the rates its _quantities, to float64 rounding (the integrand a_m - c_m is a few u53 of noise)"""
    rng = np.random.default_rng(3)
    u = rng.standard_normal((6, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    ur = u @ noe.frame_matrix(FRAME).T
    R, F = 2, 40
    res = oracle_modes(np.broadcast_to(signals(ur), (R, F, 6, 5)))
    RObj, fDD, fCSA, tf, gr = constants(600.0)
    for D in TENSORS:
        Jw = modes.J(res, D, RObj.omega, 2.0, stop=stop)
        want = eo.J_closed(RObj.omega, ur, D, 1.0, [], [])
        assert np.max(np.abs(Jw / want - 1.0)) <= 1e-13
        rel = modes.relaxation(res, D, 2.0, 600.0, stop=stop)
        q = eo._quantities(want, fDD, fCSA, tf, gr)
        for k, name in enumerate(('R1', 'R2', 'NOE')):
            assert np.max(np.abs(rel[name] / q[:, k] - 1.0)) <= 1e-12, name
        assert np.array_equal(rel['omega'], RObj.omega)


def test_sphere_gives_the_isotropic_model_free_J():
    """D = (1, 1, 1) / (6 tau_c) and a sampled C(t) = S2 + (1 - S2) exp(-t / tau_e): the isotropic J of the same function truncated at
    T = L h, within the interpolation bound h^2 / 8 max|f''| int_0^T exp(-E t) dt, f = (1 - S2) exp(-t / tau_e)"""
    tau_c, tau_e, S2, h, L = 8000.0, 60.0, 0.7, 2.0, 400
    u = np.array([[0.3, -0.5, 0.81]])
    u /= np.linalg.norm(u)
    s = signals(u)[0]
    H1 = np.array([s[0] * s[0], s[1] * s[1], s[0] * s[1], s[2] * s[2], s[3] * s[3], s[4] * s[4]])
    k = np.arange(L + 1)
    res = dict(H=(S2 + (1 - S2) * np.exp(-k * h / tau_e))[:, None, None] * H1[None, None, :], smean=np.sqrt(S2) * s[None, :])
    D = np.ones(3) / (6.0 * tau_c)
    RObj = constants(600.0)[0]
    om = RObj.omega
    E = 1.0 / tau_c
    T = L * h
    zz = E + 1.0 / tau_e + 1j * om
    want = S2 * E / (E * E + om * om) + (1 - S2) * ((1.0 - np.exp(-zz * T)) / zz).real
    bound = h * h / 8.0 * (1 - S2) / tau_e ** 2 * (1.0 - np.exp(-E * T)) / E
    got = modes.J(res, D, om, h, stop='end')[0]
    print('sphere: |dJ| %s bound %.3e' % (np.abs(got - want), bound))
    assert np.all(np.abs(got - want) <= bound + 1e-13 * np.abs(want))
    assert np.max(np.abs(got - want)) > 0.01 * bound          # the bound is not slack by orders of magnitude
    # 'crossing' ends nowhere on a function that stays above its plateau
    assert np.max(np.abs(modes.J(res, D, om, h, stop='crossing')[0] - got)) <= 1e-13 * np.max(got)


def test_crossing_stops_where_the_function_meets_its_plateau():
    """one mode alive (u along z: only H0), a_m - c_m = 1, 0.5, -0.5, ...: the integral is the first piece plus the triangle up to the
    crossing at 1.5 h"""
    H = np.zeros((5, 1, 6))
    y = np.array([1.0, 0.5, -0.5, 0.3, 0.2])
    H[:, 0, 0] = (0.2 + y) * 4.0 / 9.0
    res = dict(H=H, smean=np.array([[np.sqrt(0.2) * 2.0 / 3.0, 0, 0, 0, 0]]))
    D = TENSORS[0]
    a, c, E = modes.amplitudes(res, D)
    m = int(np.argmax(a[0, 0]))
    assert np.allclose(a[:, 0, m] - c[0, m], y, rtol=0, atol=1e-14)
    h, om = 3.0, np.array([0.0, 0.01])
    z = E[m] + 1j * om
    t = np.array([0.0, h, 1.5 * h])
    want = c[0, m] * E[m] / (E[m] ** 2 + om ** 2) + np.array([quad_transform_nodes(t, [1.0, 0.5, 0.0], zz) for zz in z])
    got = modes.J(res, D, om, h, stop='crossing')[0]
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


def quad_transform_nodes(t, f, z):
    return integrate.quad(lambda x: np.interp(x, t, f) * np.exp(-z.real * x) * np.cos(z.imag * x), 0.0, t[-1], points=list(t[1:-1]),
                          epsabs=0.0, epsrel=1e-13)[0]


def test_bad_arguments():
    res = oracle_modes(np.zeros((1, 4, 2, 5)))
    with pytest.raises(ValueError):
        modes.J(res, TENSORS[0], [0.0], 1.0, stop='never')
    with pytest.raises(ValueError):
        modes.J(res, (1.0, -1.0, 1.0), [0.0], 1.0)
    with pytest.raises(ValueError):
        modes.J(res, TENSORS[0], [0.0], 0.0)
    with pytest.raises(ValueError):
        modes.amplitudes(dict(H=np.zeros((3, 2, 5)), smean=np.zeros((2, 5))), TENSORS[0])


# ---- the command line -----------------------------------------------------------------------------------------------------------
def test_cli_mode_flag_refusals_without_gpu(tmp_path):
    """the --mode* flags that do not fit together: the script's '= = = ERROR:' message and exit status 1 before any GPU work: the input
    file does not even exist"""
    script = os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')
    base = [sys.executable, script, '-s', 'none.pdb', '-f', str(tmp_path / 'missing.npz'), '-o', str(tmp_path / 'o')]
    full = ['--modeCt', '--tau', '100']
    cases = [(['--tau', '100', '--modeD', '1e7 1.3'], '--modeD belongs to --modeCt'),
             (['--tau', '100', '--modeField', '600'], '--modeField belongs to --modeCt'),
             (['--modeCt'], '--modeCt needs --tau'),
             (full + ['--modeField', '600'], '--modeField needs --modeD'),
             (full + ['--modeD', '1e7'], '--modeD must be'),
             (full + ['--modeD', '1e7 x'], '--modeD must be'),
             (full + ['--modeD', '-1e7 1.3'], '--modeD must be'),
             (full + ['--modeD', '1e7 1.3 12.0'], '--modeD must be'),
             (full + ['--modeD', '1e7 1.3', '--modeField', '-600'], '--modeField must be'),
             (full + ['--vecRot', '1 0 0'], '--modeCt takes --vecRot'),
             (full + ['--vecRot', '1 1 0 0'], '--modeCt takes --vecRot')]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for extra, msg in cases:
        p = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
        err = p.stderr.decode()
        assert p.returncode == 1 and ('= = = ERROR: ' in err) and msg in err, (extra, p.returncode, err[-500:])
        assert not os.listdir(str(tmp_path))


def test_signatures_present():
    from spinrelax_amd import _lib
    for name in ('sr_ct_modes_max_frames', 'sr_pack_modes_f32_dev', 'sr_ct_modes_f32_dev', 'sr_vectors_ct_modes_f32'):
        assert name in _lib.SIGNATURES
