"""
Pins the CPU oracle (oracle/sr_oracle.py, oracle/ct_palmer_oracle.c) against the golden vectors the
REAL reference produced in the build container (oracle/gen_golden.py).  CPU only.
"""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT, golden, relerr
import sr_oracle as o
from spinrelax_amd import synth


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope='module')
def liboracle():
    so = os.path.join(ROOT, 'oracle', 'libsr_oracle.so')
    if not os.path.isfile(so):
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'oracle'), 'libsr_oracle.so'])
    lib = ctypes.CDLL(so)
    lib.sr_oracle_ct_palmer_f64.restype = ctypes.c_int
    return lib


def c_oracle_ct(lib, v4):
    v4 = np.ascontiguousarray(v4, dtype=np.float32)
    R, F, V, _ = v4.shape
    L = F // 2
    Ct = np.empty((L, V))
    dCt = np.empty((L, V))
    rc = lib.sr_oracle_ct_palmer_f64(v4.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(R), ctypes.c_int64(F),
                                     ctypes.c_int64(V), Ct.ctypes.data_as(ctypes.c_void_p),
                                     dCt.ctypes.data_as(ctypes.c_void_p), None)
    assert rc == 0
    return Ct, dCt


@pytest.mark.parametrize('tag,cfg,nvec', [('cfg1', 1, None), ('cfg2', 2, None), ('cfg3s', 3, 8)])
def test_synth_is_bit_reproducible(tag, cfg, nvec, synth_cache):
    g = golden('%s_ct.npz' % tag)
    assert sha(synth_cache(cfg, nvec)) == str(g['input_sha'])


def test_ct_numpy_oracle_vs_reference_cfg1(synth_cache):
    g = golden('cfg1_ct.npz')
    s = synth.config_shapes(1)
    v4 = o.reformat_vecs_by_tau([synth_cache(1)], s['dt'], s['tau_memory'])
    assert v4.shape == (s['R'], s['F'], s['V'], 3)
    np.testing.assert_array_equal(o.calculate_dt(s['dt'], s['tau_memory']), g['t'])
    Ct, dCt = o.calculate_Ct_Palmer(v4)
    # same numpy calls in the same order as the reference: bit-identical
    np.testing.assert_array_equal(Ct, g['Ct64'])
    np.testing.assert_array_equal(dCt, g['dCt64'])
    Ct32, dCt32 = o.calculate_Ct_Palmer(v4, dtype=np.float32)
    np.testing.assert_array_equal(Ct32, g['Ct32'])
    np.testing.assert_array_equal(dCt32, g['dCt32'])
    # explicit-loop and FFT formulations agree with the reference to rounding
    p = o.calculate_Ct_Palmer_perchunk(v4)
    assert relerr(p.mean(axis=0), g['Ct64']) < 1e-13
    Cf, dCf = o.calculate_Ct_fft(v4)
    assert relerr(Cf, g['Ct64']) < 1e-11
    assert relerr(dCf, g['dCt64']) < 1e-8


@pytest.mark.parametrize('tag,cfg,nvec', [('cfg1', 1, None), ('cfg2', 2, None), ('cfg3s', 3, 8)])
def test_ct_c_oracle_vs_reference(tag, cfg, nvec, synth_cache, liboracle):
    g = golden('%s_ct.npz' % tag)
    s = synth.config_shapes(cfg)
    v4 = o.reformat_vecs_by_tau([synth_cache(cfg, nvec)], s['dt'], s['tau_memory'])
    Ct, dCt = c_oracle_ct(liboracle, v4)
    assert relerr(Ct, g['Ct64']) < 1e-12
    assert relerr(dCt, g['dCt64']) < 1e-9
    # the reference's own float32 result differs from its float64 evaluation at the 1e-6 level
    # (2.6e-6) -- documents why parity is defined against the float64 evaluation
    assert relerr(g['Ct32'], g['Ct64']) < 2e-5


def test_reformat_drops_tail_per_file():
    a = np.arange(7 * 2 * 3, dtype=np.float32).reshape(7, 2, 3)
    b = 100 + np.arange(5 * 2 * 3, dtype=np.float32).reshape(5, 2, 3)
    out = o.reformat_vecs_by_tau([a, b], 1.0, 3.0)           # F = 3: keeps 6 of 7 and 3 of 5 frames
    assert out.shape == (3, 3, 2, 3)
    np.testing.assert_array_equal(out.reshape(9, 2, 3), np.concatenate([a[:6], b[:3]]))


@pytest.mark.parametrize('tag,cfg', [('cfg1', 1), ('cfg2', 2)])
def test_vec_stage_vs_reference(tag, cfg, synth_cache):
    g = golden('%s_vec.npz' % tag)
    s = synth.config_shapes(cfg)
    v4 = o.reformat_vecs_by_tau([synth_cache(cfg)], s['dt'], s['tau_memory'])
    v3 = v4.reshape(-1, s['V'], 3)
    rot = o.rotate_vector_simd(v3, g['q'])
    assert rot.dtype == np.float64
    np.testing.assert_array_equal(rot[g['rot_idx_n'], g['rot_idx_v']], g['rot_sample'])
    hist, edges = o.lambert_histogram(rot)
    np.testing.assert_array_equal(hist.astype(np.uint32), g['hist'])
    np.testing.assert_array_equal(edges[0], g['edges_phi'])
    np.testing.assert_array_equal(edges[1], g['edges_cos'])
    np.testing.assert_array_equal(o.lambert_edges()[0], g['edges_phi'])
    np.testing.assert_array_equal(o.lambert_edges()[1], g['edges_cos'])
    assert hist.sum() == g['hist_sum']
    np.testing.assert_array_equal(o.mean_vector(rot), g['avgvec'])
    np.testing.assert_array_equal(o.calculate_S2_by_outerProduct(rot, s['dt'], s['tau_memory']), g['S2_tau'])
    np.testing.assert_array_equal(o.calculate_S2_by_outerProduct(rot), g['S2_all'])


@pytest.mark.parametrize('tag,nres', [('cfg1', 32), ('cfg2', 16), ('cfg3s', 8)])
def test_fit_vs_reference(tag, nres):
    g = golden('%s_fit.npz' % tag)
    assert len(g['names']) == nres
    orders = list(g['listDoG'])
    for i in range(nres if tag == 'cfg1' else min(nres, 4)):
        t, y, dy = g['t'][i], g['y'][i], g['dy'][i]
        best, trials = o.optimised_curve_fitting(t, y, dy, listDoG=orders)
        for fit in trials:
            j = orders.index(fit['nParams'])
            nP = fit['nParams']
            np.testing.assert_array_equal(fit['p0'], g['trial_p0'][i, j, :nP])
            assert list(fit['quality']) == list(g['trial_quality'][i, j])
            assert fit['chiSq'] == g['trial_chi'][i, j]
        assert best is not None
        assert best['nParams'] == g['sel_nParams'][i]
        K = best['nParams'] // 2
        assert best['chiSq'] == g['sel_chi'][i]
        np.testing.assert_array_equal(best['C'], g['sel_C'][i, :K])
        np.testing.assert_array_equal(best['tau'], g['sel_tau'][i, :K])
        np.testing.assert_array_equal(best['dC'], g['sel_dC'][i, :K])
        np.testing.assert_array_equal(best['dtau'], g['sel_dtau'][i, :K])
        assert best['S2'] == g['sel_S2'][i]
        assert best['dS2'] == g['sel_dS2'][i]


def _params(g):
    n = len(g['names'])
    K = g['nComps']
    zeta = float(g['zeta'])
    S2 = [zeta * g['S2'][i] for i in range(n)]
    C = [zeta * g['C'][i, :K[i]] for i in range(n)]
    tau = [g['tau'][i, :K[i]] for i in range(n)]
    return n, S2, C, tau


def test_relax_old_api_vs_reference():
    g = golden('cfg1_relax.npz')
    n, S2, C, tau = _params(g)
    Dpar, Dperp = o.symmtop_from_iso(float(g['Diso']), float(g['Dani']))
    bv = np.repeat(g['binvecs'][None], n, axis=0)
    for fi, MHz in enumerate(g['fields']):
        B0 = o.B0_from_Hz(MHz * 1e6)
        np.testing.assert_array_equal(o.omega_set(B0, 'ps'), g['omega_%d' % fi])
        iso = o.obtain_R1R2NOErho('rigid_sphere', float(g['Diso']), B0, S2, C, tau)
        np.testing.assert_array_equal(iso, g['iso_f32_%d' % fi])
        iso64 = o.obtain_R1R2NOErho('rigid_sphere', float(g['Diso']), B0, S2, C, tau, cast32=False)
        assert relerr(iso64, g['iso_f64_%d' % fi]) < 1e-14
        J = np.array([o.J_combine_isotropic_exp_decayN(o.omega_set(B0), 1.0 / (6.0 * float(g['Diso'])), S2[i], C[i], tau[i])
                      for i in range(n)])
        np.testing.assert_array_equal(J, g['iso_J_%d' % fi])
        for nm, csa in (('sym', None), ('symcsa', g['csa_alt'])):
            sym = o.obtain_R1R2NOErho('rigid_symmtop', (Dpar, Dperp), B0, S2, C, tau, vecXH=bv, weights=g['weights'], csa=csa)
            np.testing.assert_array_equal(sym, g['%s_f32_%d' % (nm, fi)])
            sym64 = o.obtain_R1R2NOErho('rigid_symmtop', (Dpar, Dperp), B0, S2, C, tau, vecXH=bv, weights=g['weights'],
                                        csa=csa, cast32=False)
            assert relerr(sym64, g['%s_f64_%d' % (nm, fi)]) < 1e-13
        Jm = o.J_combine_symmtop_exp_decayN(o.omega_set(B0), g['binvecs'], Dpar, Dperp, S2[0], C[0], tau[0])
        np.testing.assert_array_equal(Jm, g['sym_J_res0_%d' % fi])
        one = o.obtain_R1R2NOErho('rigid_symmtop', (Dpar, Dperp), B0, S2, C, tau, vecXH=g['sym1_vecs'])
        np.testing.assert_array_equal(one, g['sym1_f32_%d' % fi])


def test_relax_new_api_vs_reference():
    g = golden('cfg1_relax.npz')
    n = len(g['names'])
    K = g['nComps']
    S2 = list(g['S2'])
    C = [g['C'][i, :K[i]] for i in range(n)]
    tau = [g['tau'][i, :K[i]] for i in range(n)]
    for fi, MHz in enumerate(g['fields']):
        om, B0 = o.omega_set_new(MHz)
        np.testing.assert_array_equal(om, g['new_omega_%d' % fi])
        for kind in ('R1', 'R2', 'NOE'):
            v, e = o.new_api_eval(kind, MHz, float(g['Diso']), float(g['Dani']), S2, C, tau, float(g['zeta']),
                                  g['binvecs'], g['weights'], -170e-6)
            assert relerr(v, g['new_%s_val_%d' % (kind, fi)]) < 1e-13
            assert relerr(e, g['new_%s_err_%d' % (kind, fi)]) < 1e-10
    assert o.factor_DD_new() == float(g['new_fDD'])


def test_histogram_to_vectors():
    g = golden('cfg1_relax.npz')
    v = golden('cfg1_vec.npz')
    hist = v['hist'].astype(np.float64)
    bv, w = o.convert_LambertCylindricalHist_to_vecs(hist, [v['edges_phi'], v['edges_cos']])
    np.testing.assert_array_equal(bv[0], g['binvecs'])
    np.testing.assert_array_equal(w, g['weights'])


def test_known_answers():
    k = json.load(open(os.path.join(GOLD, 'known_answers.json')))
    assert o.factor_DD_new() == k['f_DD']
    assert abs(k['f_DD'] - 519627720.1974593) < 1e-6          # spectral_densities.py:2189
    assert abs(o.factor_DD() / k['f_DD'] - 1) < 3e-16           # old API: gamma order differs by 1 ulp
    B0 = o.B0_from_Hz(600.133e6)
    np.testing.assert_array_equal(o.omega_set(B0, 'ps'), k['omega_600_133_ps'])
    rs = k['rigid_sphere']
    J = o.J_combine_isotropic_exp_decayN(o.omega_set(B0), 1.0 / (6.0 * rs['Diso']), rs['S2'], [0.], [99999.])
    R1, R2, NOE = o.relax_from_J(J, B0, -170e-6, 1e-12)
    assert (R1, R2, NOE) == (rs['R1'], rs['R2'], rs['NOE'])
    # BASELINE.md known answers
    assert abs(R1 - 2.216697349136826) < 1e-14 and abs(R2 - 6.743109911585374) < 1e-14
    assert abs(NOE - 0.7864966280916813) < 1e-15
    jo = k['Jomega_outer']
    out = o.Jomega(np.array(jo['x'])[:, None], np.array(jo['y'])[None, :])
    np.testing.assert_array_equal(out, np.array(jo['out']))


def test_oracle_pinned_against_live_reference_when_present(synth_cache):
    """In the build container the real reference is importable: run both live on a fresh seed."""
    import ref_loader
    if not ref_loader.available():
        pytest.skip('reference not present (GPU box)')
    import contextlib
    import io
    ref = ref_loader.load()
    v = synth.synth_vectors(600, 5, seed=77)
    with contextlib.redirect_stdout(io.StringIO()):
        v4r = ref.calcCt.reformat_vecs_by_tau([v], 10.0, 1200.0)
        Cr, dCr = ref.calcCt.calculate_Ct_Palmer(v4r.astype(np.float64))
    v4 = o.reformat_vecs_by_tau([v], 10.0, 1200.0)
    np.testing.assert_array_equal(v4, v4r)
    Co, dCo = o.calculate_Ct_Palmer(v4)
    np.testing.assert_array_equal(Co, Cr)
    np.testing.assert_array_equal(dCo, dCr)
    q = np.array([0.3, -0.5, 0.1, 0.8])
    np.testing.assert_array_equal(o.rotate_vector_simd(v, q), ref.qs.rotate_vector_simd(v, q))


def test_oracle_per_frame_rotation_equals_reference():
    """rotate_vector_simd with one quaternion per frame: the oracle's broadcast form against
    the reference run bond by bond (the only N-D form the reference's own broadcasting supports)."""
    g = golden('cfg1_detumble.npz')
    qinv = g['q32'].astype(np.float64)
    qinv[:, 1:] *= -1.0
    back = o.rotate_vector_simd(g['lab'][:, :8], qinv[:, None, :])
    assert back.dtype == np.float64
    np.testing.assert_array_equal(back, g['body64'])
    s = dict(dt=10.0, tau=1000.0)
    full = o.rotate_vector_simd(g['lab'], qinv[:, None, :]).astype(np.float32)
    v4 = o.reformat_vecs_by_tau([full], s['dt'], s['tau'])
    Ct, dCt = o.calculate_Ct_Palmer(v4.astype(np.float64))
    np.testing.assert_array_equal(Ct, g['Ct64'])
    np.testing.assert_array_equal(dCt, g['dCt64'])


def test_fit_eval_reference_step_rule_and_quotient():
    """The host reference of the fit-evaluation tests (tests/test_gpu_fit_eval.py): fd_step_2point is scipy's own step rule
    (optimize/_numdiff.py: _compute_absolute_step + _adjust_scheme_to_bounds '1-sided'), bit for bit, for x inside, on and within a
    step of the bounds; expfit_eval_exact's 80-bit forward quotient of a cfg2 fixture residue agrees with scipy's float64
    approx_derivative to the forward-difference noise of float64 (rounding of f over dx), and its analytic Jacobian with the model."""
    from scipy.optimize import _numdiff
    rng = np.random.default_rng(11)
    tau_max = 51200.0
    lb, ub = np.zeros(5), np.array([1.0, 1.0, tau_max, tau_max, 1.0])
    xs = [rng.uniform(lb, ub) for _ in range(50)]
    xs += [np.array([0.0, 1.0, tau_max, 1e-300, 0.0]), np.array([1 - 1e-9, 1e-9, tau_max * (1 - 1e-12), 5e-324, 1.0]),
           np.array([0.5, 0.5, 1.0, 0.999999999, 1 - 2e-8])]
    for x in xs:
        h0 = _numdiff._compute_absolute_step(None, x, np.zeros(3), '2-point')
        h_ref, _ = _numdiff._adjust_scheme_to_bounds(x, h0, 1, '1-sided', lb, ub)
        h, dx = o.fd_step_2point(x, lb, ub)
        assert np.array_equal(h, h_ref), (x, h, h_ref)
        assert np.array_equal(dx, (x + h_ref) - x)
    g = golden('cfg2_fit.npz')
    t, y, dy = g['t'][0], g['y'][0], g['dy'][0]
    x = g['trial_popt'][0, 2, :5]
    lb5, ub5 = np.zeros(5), np.array([1.0, 1.0, t[-1] * 10, t[-1] * 10, 1.0])
    ex = o.expfit_eval_exact(t, y, 1.0 / dy, x, lb5, ub5, 0)

    def fun(p):
        return (o.curvefit_exponential(t, *p) - y) / dy
    J64 = _numdiff.approx_derivative(fun, x, method='2-point', bounds=(lb5, ub5))
    J = np.asarray(ex['J'], dtype=np.float64)
    noise = 8 * np.finfo(float).eps * np.max(np.abs(fun(x)) + np.abs(y / dy)) / np.abs(ex['dx'])
    assert np.all(np.abs(J64 - J) <= noise[None, :] + 1e-12 * np.abs(J)), np.max(np.abs(J64 - J) / noise[None, :])
    an = o.expfit_eval_exact(t, y, 1.0 / dy, x, lb5, ub5, 1)
    assert np.max(np.abs(np.asarray(an['f'], dtype=np.float64) - fun(x))) < 1e-14 * np.max(np.abs(y / dy))   # f cancels: absolute
    e = np.exp(-t / x[2])
    assert relerr(np.asarray(an['J'][:, 2], dtype=np.float64), x[0] * e * t / x[2] ** 2 / dy) < 1e-12
