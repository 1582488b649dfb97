"""
CPU tests of the host side of the fully anisotropic (rhombic) diffusion model: the helpers of spinrelax_amd/_hostmath.py against
the two numpy oracles of tests/ellipsoid_oracle.py (closed form, and the independent l = 2 operator form), the
(Diso, aniso, rhomb) <-> (Dx, Dy, Dz) conversion, and diffusionModel's unit / Diso handling.  No GPU, no library.
"""
import numpy as np
import pytest

from conftest import relerr
import ellipsoid_oracle as eo
from spinrelax_amd import _hostmath as hm

DISO = 1.2e-5           # ps^-1, a small protein
OMEGA = np.array([0.0, 3.8e-4, 3.39e-3, 3.77e-3, 4.15e-3])      # [0, wN, wH-wN, wH, wH+wN] at 600 MHz, ps^-1
TENSORS = [hm.ellipsoid_from_iso(DISO, 1.26, 0.4), hm.ellipsoid_from_iso(DISO, 0.8, 0.3), hm.ellipsoid_from_iso(DISO, 1.6, 1.0),
           (0.7e-5, 1.9e-5, 1.1e-5), (2.0e-5, 1.0e-5, 0.6e-5)]


def unit_vectors(n, seed=0):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    v = np.concatenate((v, np.identity(3), [[0.6, 0.8, 0.0], [0.0, -0.6, 0.8]]))
    return v / np.linalg.norm(v, axis=1)[:, None]


def test_oracle_forms_agree_with_each_other():
    """the two oracle forms themselves: closed form against the operator form"""
    v = unit_vectors(200)
    for D in TENSORS:
        a = eo.J_closed(OMEGA, v, D, 0.8, [0.05, 0.1], [40.0, 1500.0])
        b = eo.J_operator(OMEGA, v, D, 0.8, [0.05, 0.1], [40.0, 1500.0])
        assert relerr(a, b) < 1e-12
        np.testing.assert_allclose(np.sort(eo.rates_closed(D)[0]), np.linalg.eigvalsh(
            sum(d * (L @ L) for d, L in zip(D, eo._l2_matrices()))), rtol=1e-13)


@pytest.mark.parametrize('D', TENSORS)
def test_host_helpers_vs_both_oracles(D):
    v = unit_vectors(200, seed=1)
    assert relerr(hm.D_coefficients_ellipsoid(D), eo.rates_closed(D)[0]) < 1e-12
    A = hm.A_coefficients_ellipsoid(v, D)
    assert A.shape == (v.shape[0], 5)
    assert np.max(np.abs(A.sum(axis=-1) - 1.0)) < 1e-14
    assert np.max(np.abs(A - eo.amplitudes_closed(v, D))) < 1e-12          # amplitudes are O(1); some are exactly 0
    for S2, C, tau in ((0.85, [], []), (0.7, [0.19], [55.0]), (0.5, [0.02, 0.03, 0.05, 0.1], [3.0, 30.0, 300.0, 3000.0])):
        J = hm.J_combine_ellipsoid_exp_decayN(OMEGA, v, D, S2, C, tau)
        assert J.shape == (v.shape[0], 5)
        assert relerr(J, eo.J_closed(OMEGA, v, D, S2, C, tau)) < 1e-12
        assert relerr(J, eo.J_operator(OMEGA, v, D, S2, C, tau)) < 1e-12


def test_amplitudes_over_leading_dimensions():
    v = unit_vectors(19, seed=2).reshape(4, 6, 3)
    D = TENSORS[0]
    A = hm.A_coefficients_ellipsoid(v, D)
    assert A.shape == (4, 6, 5)
    np.testing.assert_array_equal(A[2, 3], hm.A_coefficients_ellipsoid(v[2, 3], D))
    J = hm.J_combine_ellipsoid_exp_decayN(OMEGA, v, D, 0.8, [0.1], [100.0])
    assert J.shape == (4, 6, 5)


def test_limits_symmetric_top_sphere_and_permutation():
    v = unit_vectors(50, seed=3)
    S2, C, tau = 0.8, [0.1], [200.0]
    for aniso, prolate in ((1.26, True), (0.8, False)):
        Dpar, Dperp = hm.symmtop_from_iso(DISO, aniso)
        D = (Dperp, Dperp, Dpar) if prolate else (Dpar, Dperp, Dperp)
        dj = hm.D_coefficients_symmtop((Dpar, Dperp))[:, None]
        G = S2 * dj / (dj * dj + OMEGA ** 2) + C[0] * (dj + 1 / tau[0]) / ((dj + 1 / tau[0]) ** 2 + OMEGA ** 2)
        ref = hm.A_coefficients_symmtop(v, prolate) @ G
        assert relerr(hm.J_combine_ellipsoid_exp_decayN(OMEGA, v, D, S2, C, tau), ref) < 1e-12
    # sphere: R == 0 exactly, no NaN, and no dependence on the vector
    J = hm.J_combine_ellipsoid_exp_decayN(OMEGA, v, (DISO, DISO, DISO), S2, C, tau)
    k0, k1 = 6 * DISO, 6 * DISO + 1 / tau[0]
    assert np.all(np.isfinite(J))
    assert relerr(J, np.broadcast_to(S2 * k0 / (k0 ** 2 + OMEGA ** 2) + C[0] * k1 / (k1 ** 2 + OMEGA ** 2), J.shape)) < 1e-12
    # joint permutation of axes and components
    D = np.array(TENSORS[0])
    ref = hm.J_combine_ellipsoid_exp_decayN(OMEGA, v, D, S2, C, tau)
    for perm in ([1, 2, 0], [2, 1, 0], [0, 2, 1]):
        assert relerr(hm.J_combine_ellipsoid_exp_decayN(OMEGA, v[:, perm], D[perm], S2, C, tau), ref) < 1e-12


def test_triple_conversion():
    for aniso in (1.0, 1.01, 1.26, 2.5):
        for rhomb in (0.0, 0.1, 0.4, 1.0):
            Dx, Dy, Dz = hm.ellipsoid_from_iso(DISO, aniso, rhomb)
            assert Dx <= Dy <= Dz
            assert abs((Dx + Dy + Dz) / 3.0 / DISO - 1.0) < 1e-15
            if aniso > 1.0:
                assert abs(3 * (Dy - Dx) / (2 * Dz - Dx - Dy) - rhomb) < 1e-12          # the ROTDIF rhombicity
    # round trips, prolate and oblate side, rhombicity of either sign below 1
    for aniso in (1.26, 0.8, 3.0, 0.4):
        for rhomb in (0.0, 0.25, 0.4, 0.99, -0.5):
            back = hm.iso_from_ellipsoid(hm.ellipsoid_from_iso(DISO, aniso, rhomb))
            np.testing.assert_allclose(back, (DISO, aniso, rhomb), rtol=1e-12, atol=1e-14)
    # any tensor: with the unique axis it reports, the triple gives the tensor back
    for D in TENSORS + [(10.0, 11.0, 5.0), (10.0, 8.0, 5.0), (1.0, 3.0, 1.1), (2.0, 2.0, 2.0)]:
        np.testing.assert_allclose(hm.ellipsoid_from_iso(*hm.iso_from_ellipsoid(D, with_axis=True)), D, rtol=1e-14)
    # rhomb = 0: exactly the reference's symmetric top, unique axis z (prolate) or x (oblate)
    for aniso in (1.26, 0.8):
        Dpar, Dperp = hm.symmtop_from_iso(DISO, aniso)
        D = hm.ellipsoid_from_iso(DISO, aniso, 0.0)
        assert D == ((Dperp, Dperp, Dpar) if aniso >= 1 else (Dpar, Dperp, Dperp))


def test_diffusionModel_ellipsoid():
    from spinrelax_amd import spectral_densities as sd
    m = sd.diffusionModel('rigid_ellipsoid_Dref', 'ps', DISO, 1.26, 0.4)
    assert m.name == 'rigid_ellipsoid'
    np.testing.assert_array_equal(m.D, hm.ellipsoid_from_iso(DISO, 1.26, 0.4))
    m2 = sd.diffusionModel('rigid_ellipsoid_D', 'ps', *m.D)
    np.testing.assert_array_equal(m2.D, m.D)
    m.set_time_unit('ns')                          # all three values scale: 1/ps -> 1/ns
    np.testing.assert_allclose(m.D, 1e3 * m2.D, rtol=1e-15)
    np.testing.assert_allclose(hm.iso_from_ellipsoid(m.D), (1e3 * DISO, 1.26, 0.4), rtol=1e-12)
    m.change_Diso(2.5e-2)                          # all three by one factor: anisotropy and rhombicity stay
    np.testing.assert_allclose(hm.iso_from_ellipsoid(m.D), (2.5e-2, 1.26, 0.4), rtol=1e-12)
    assert sd._model_args(type('R', (), {'rotdifModel': m})())[0] == 3


def test_class_api_rhombicity_defaults_to_symmetric_path():
    from spinrelax_amd import spectral_densities as sd
    g = sd.globalRotationalDiffusion_Axisymmetric(D=[DISO, 1.26])
    assert g.get_Drhomb() == 0.0 and g.kernel_model()[0] == 2
    g.set_Drhomb(0.4)
    model, D = g.kernel_model()
    assert model == 3 and tuple(D) == hm.ellipsoid_from_iso(DISO, 1.26, 0.4)
    e = sd.globalRotationalDiffusion_Ellipsoid(D=[DISO, 1.26, 0.0])
    assert e.kernel_model()[0] == 3                 # built from three values: the ellipsoid path, rhombicity 0 included
    e = sd.globalRotationalDiffusion_Ellipsoid(D=[2.0e-5, 1.0e-5, 0.6e-5], bConvert=True)
    np.testing.assert_allclose(e.kernel_model()[1], [2.0e-5, 1.0e-5, 0.6e-5], rtol=1e-14)
    assert 'Drhomb' in sd.spinRelaxationExperiments.listAllowedOptimisationVariables
    assert sd.spinRelaxationExperiments.dictStepSizes['Drhomb'] == 0.1
    assert sd.spinRelaxationExperiments.dictExportUnits['Drhomb'] == 'a.u.'
