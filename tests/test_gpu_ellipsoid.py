"""
GPU tests of the fully anisotropic (rhombic) rotational-diffusion model: model 3 of sr_jomega_relax_f64 (k_relax<EllipsoidCoef>,
spinrelax_amd/csrc/sr_relax.hip) against the independent l = 2 operator-form oracle of tests/ellipsoid_oracle.py, its limits
against the existing models 1 and 2 on the same inputs, the three-value -D of calculate-relaxations-from-Ct.py, the rsCSA search
on model-3 statistics and the global Drhomb optimisation of the class API.

Bars: J and the table means 1e-12 relative (the bar of the symmetric-top J comparison, test_gpu_parity.py); sigmas 1e-8 relative
(the bar of the symmetric-top sigma comparison there and in test_gpu_multifield.py) next to an absolute floor of 1e-14 |mean|:
a sigma is the root of a mean of squared DIFFERENCES of values that each carry a few ulp of |mean|, so where the distribution
has no width (one bin, the sphere) the true sigma is 0 and what is left is that rounding, not a relative quantity.
"""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT, files_equal_numeric, golden, relerr
import ellipsoid_oracle as eo
from spinrelax_amd import synth
from spinrelax_amd import _hostmath as hm
from spinrelax_amd import general_scripts as gs
from spinrelax_amd import fitting_Ct_functions as fitCt
from spinrelax_amd import spectral_densities as sd

pytestmark = pytest.mark.gpu
SCR = os.path.join(ROOT, 'scripts')
DISO = 3.7e-5
D_RHOMBIC = hm.ellipsoid_from_iso(DISO, 1.26, 0.4)
NRES = 3


@pytest.fixture(scope='module')
def ctx():
    from spinrelax_amd.hip import Context
    c = Context(0)
    yield c
    c.close()


def sigma_close(got, ref, mean):
    return bool(np.all(np.abs(got - ref) <= 1e-8 * np.abs(ref) + 1e-14 * np.abs(mean)))


def table_close(got, ref):
    """(…, 2) tables of [mean, sigma]"""
    return relerr(got[..., 0], ref[..., 0]) < 1e-12 and sigma_close(got[..., 1], ref[..., 1], ref[..., 0])


def stats_close(got, ref):
    """[a1, b1, Var a1, Cov(a1,b1), Var b1, a2, b2, Var a2, Cov(a2,b2), Var b2, N, Var N]: means 1e-12; second moments to the
    square of the sigma bar's terms, 2e-8 relative next to (1e-14 |mean|)^2-sized floors built from the means they belong to"""
    ok = relerr(got[..., [0, 1, 5, 6, 10]], ref[..., [0, 1, 5, 6, 10]]) < 1e-12
    for k, (m1, m2) in {2: (0, 0), 3: (0, 1), 4: (1, 1), 7: (5, 5), 8: (5, 6), 9: (6, 6), 11: (10, 10)}.items():
        floor = 1e-14 * np.abs(ref[..., m1] * ref[..., m2])          # sigma_1 sigma_2 <= |m1 m2|: the floor of one factor
        ok = ok and bool(np.all(np.abs(got[..., k] - ref[..., k]) <= 2e-8 * np.abs(ref[..., k]) + floor))
    return ok


def two_fields(n):
    af = [sd.angularFrequencies(fieldStrength=f) for f in (600.133, 800.0)]
    om = np.array([a.omega for a in af])
    fdd = np.array([a.get_factor_DD() for a in af])
    csa = np.linspace(-160e-6, -180e-6, n)
    fcsa = np.array([2.0 / 15.0 * csa ** 2 * (a.gA.gamma * a.B0) ** 2 for a in af])
    return om, fdd, fcsa, 1e-12, af[0].gB.gamma / af[0].gA.gamma


def three_residues():
    """K = 0, 1 and 8 components in one launch"""
    S2 = np.array([0.85, 0.7, 0.45])
    C = np.zeros((NRES, 8))
    tau = np.ones((NRES, 8))
    C[1, 0], tau[1, 0] = 0.19, 55.0
    C[2] = [0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09]
    tau[2] = [2.0, 7.0, 25.0, 90.0, 300.0, 1100.0, 4000.0, 15000.0]
    return S2, C, tau, np.array([0, 1, 8], dtype=np.int32)


def bin_vectors(B, seed=0):
    if B == 2592:               # the Lambert histogram of the pipeline, 72 x 36
        return hm.lambert_bin_vectors([np.linspace(-np.pi, np.pi, 73), np.linspace(-1.0, 1.0, 37)])
    v = np.random.default_rng(seed + B).normal(size=(B, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def bin_weights(B, seed=0):
    w = np.random.default_rng(100 + seed + B).integers(0, 40, size=(NRES, B)).astype(float)
    w[:, ::7] = 0.0             # empty bins
    w[:, B // 2] = 11.0         # never all of them (B = 1: the one bin)
    return w


@pytest.mark.parametrize('noe_mode', [0, 1])
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('B', [1, 255, 257, 2592])
def test_kernel_vs_operator_oracle(ctx, B, weighted, noe_mode):
    om, fdd, fcsa, tf, gr = two_fields(NRES)
    S2, C, tau, K = three_residues()
    bv = bin_vectors(B)
    w = bin_weights(B) if weighted else None
    out, J, st = ctx.relax(3, D_RHOMBIC, om, fdd, fcsa, tf, gr, S2, C, tau, K, binvecs=bv, weights=w, noe_mode=noe_mode,
                           want_J=True, want_stats=True)
    rout, rJ, rst = eo.relax_table(D_RHOMBIC, om, fdd, fcsa, tf, gr, S2, C, tau, K, bv, w, noe_mode=noe_mode)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(J)) and np.all(np.isfinite(st))
    assert table_close(out, rout), (relerr(out[..., 0], rout[..., 0]), out[..., 1], rout[..., 1])
    assert table_close(J, rJ), (relerr(J[..., 0], rJ[..., 0]), J[..., 1], rJ[..., 1])
    assert stats_close(st, rst), (st, rst)
    if B > 1:
        assert np.all(out[..., 1] > 0)              # a real distribution: the sigmas are not the floor


def test_kernel_one_vector_per_residue(ctx):
    om, fdd, fcsa, tf, gr = two_fields(NRES)
    S2, C, tau, K = three_residues()
    v = bin_vectors(NRES, seed=5)
    for noe_mode in (0, 1):
        out, J, st = ctx.relax(3, D_RHOMBIC, om, fdd, fcsa, tf, gr, S2, C, tau, K, resvecs=v, noe_mode=noe_mode, want_J=True,
                               want_stats=True)
        rout, rJ, rst = eo.relax_table(D_RHOMBIC, om, fdd, fcsa, tf, gr, S2, C, tau, K, v, per_residue=True, noe_mode=noe_mode)
        assert relerr(out[..., 0], rout[..., 0]) < 1e-12 and np.all(out[..., 1] == 0)
        assert relerr(J[..., 0], rJ[..., 0]) < 1e-12 and np.all(J[..., 1] == 0)
        assert relerr(st[..., [0, 1, 5, 6, 10]], rst[..., [0, 1, 5, 6, 10]]) < 1e-12
        assert np.all(st[..., [2, 3, 4, 7, 8, 9, 11]] == 0)


def test_binding_errors(ctx):
    om, fdd, fcsa, tf, gr = two_fields(NRES)
    S2, C, tau, K = three_residues()
    with pytest.raises(ValueError):
        ctx.relax(3, D_RHOMBIC[:2], om, fdd, fcsa, tf, gr, S2, C, tau, K, binvecs=bin_vectors(8))
    with pytest.raises(ValueError):
        ctx.relax(3, D_RHOMBIC, om, fdd, fcsa, tf, gr, S2, C, tau, K)
    from spinrelax_amd._lib import SpinRelaxHipError
    with pytest.raises(SpinRelaxHipError, match='model must be 0, 1, 2 or 3'):
        ctx.relax(4, D_RHOMBIC, om, fdd, fcsa, tf, gr, S2, C, tau, K, binvecs=bin_vectors(8))


# ---- limits: model 3 against the existing models on the same inputs --------------------------------------------------------
def _both(ctx, model_a, D_a, D_b, bv, w, noe_mode=1):
    om, fdd, fcsa, tf, gr = two_fields(NRES)
    S2, C, tau, K = three_residues()
    kw = dict(noe_mode=noe_mode, want_J=True, want_stats=True)
    if model_a >= 2:
        a = ctx.relax(model_a, D_a, om, fdd, fcsa, tf, gr, S2, C, tau, K, binvecs=bv, weights=w, **kw)
    else:
        a = ctx.relax(model_a, D_a, om, fdd, fcsa, tf, gr, S2, C, tau, K, **kw)
    b = ctx.relax(3, D_b, om, fdd, fcsa, tf, gr, S2, C, tau, K, binvecs=bv, weights=w, **kw)
    return a, b


@pytest.mark.parametrize('aniso', [1.26, 0.8])
def test_limit_symmetric_top(ctx, aniso):
    """(Dperp, Dperp, Dpar) against model 2 prolate, (Dpar, Dperp, Dperp) against model 2 oblate (unique axis x)"""
    Dpar, Dperp = hm.symmtop_from_iso(DISO, aniso)
    D3 = (Dperp, Dperp, Dpar) if aniso > 1 else (Dpar, Dperp, Dperp)
    assert D3 == hm.ellipsoid_from_iso(DISO, aniso, 0.0)
    for noe_mode in (0, 1):
        (o2, J2, s2), (o3, J3, s3) = _both(ctx, 2, [Dpar, Dperp], D3, bin_vectors(257), bin_weights(257), noe_mode)
        assert table_close(o3, o2) and table_close(J3, J2) and stats_close(s3, s2)


def test_limit_sphere(ctx):
    (o1, J1, s1), (o3, J3, s3) = _both(ctx, 1, [DISO], (DISO, DISO, DISO), bin_vectors(257), bin_weights(257))
    assert np.all(np.isfinite(o3)) and np.all(np.isfinite(J3)) and np.all(np.isfinite(s3))
    assert table_close(o3, o1) and table_close(J3, J1) and stats_close(s3, s1)


def test_limit_tiny_rhombicity(ctx):
    bv, w = bin_vectors(257), bin_weights(257)
    (_, _, _), (o0, J0, s0) = _both(ctx, 2, list(hm.symmtop_from_iso(DISO, 1.26)), hm.ellipsoid_from_iso(DISO, 1.26, 0.0), bv, w)
    (_, _, _), (o9, J9, s9) = _both(ctx, 2, list(hm.symmtop_from_iso(DISO, 1.26)), hm.ellipsoid_from_iso(DISO, 1.26, 1e-9), bv, w)
    assert np.all(np.isfinite(o9)) and np.all(np.isfinite(J9)) and np.all(np.isfinite(s9))
    assert relerr(o9[..., 0], o0[..., 0]) < 1e-8 and relerr(J9[..., 0], J0[..., 0]) < 1e-8
    assert np.all(np.abs(o9[..., 1] - o0[..., 1]) <= 1e-8 * np.abs(o0[..., 0]))
    # and the nearly spherical tensor, where Diso^2 - L^2 is a difference of nearly equal numbers
    D = hm.ellipsoid_from_iso(DISO, 1.0 + 1e-9, 0.5)
    (o1, J1, _), (o3, J3, s3) = _both(ctx, 1, [DISO], D, bv, w)
    assert np.all(np.isfinite(o3)) and np.all(np.isfinite(J3)) and np.all(np.isfinite(s3))
    assert relerr(o3[..., 0], o1[..., 0]) < 1e-8 and relerr(J3[..., 0], J1[..., 0]) < 1e-8


def test_joint_permutation_of_axes_and_vectors(ctx):
    bv, w = bin_vectors(257), bin_weights(257)
    D = np.array(D_RHOMBIC)
    om, fdd, fcsa, tf, gr = two_fields(NRES)
    S2, C, tau, K = three_residues()
    ref = ctx.relax(3, D, om, fdd, fcsa, tf, gr, S2, C, tau, K, binvecs=bv, weights=w, noe_mode=1, want_J=True, want_stats=True)
    for perm in ([1, 2, 0], [2, 1, 0], [0, 2, 1], [1, 0, 2]):
        got = ctx.relax(3, D[perm], om, fdd, fcsa, tf, gr, S2, C, tau, K, binvecs=np.ascontiguousarray(bv[:, perm]), weights=w,
                        noe_mode=1, want_J=True, want_stats=True)
        assert table_close(got[0], ref[0]) and table_close(got[1], ref[1]) and stats_close(got[2], ref[2])


# ---- end to end: the three-value -D of calculate-relaxations-from-Ct.py ------------------------------------------------------
def run(script, *args, expect=0):
    cmd = [sys.executable, os.path.join(SCR, script)] + [str(a) for a in args]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == expect, p.stdout.decode()
    return p.stdout.decode()


CFG1 = ('-f', os.path.join(GOLD, 'cfg1_fittedCt.dat'), '--distfn', os.path.join(GOLD, 'cfg1_vecHistogram.npz'),
        '-F', '600.133e6', '--tu', 'ps', '--zeta', '0.890023')


def test_script_three_values_rhomb0_equals_two_values(tmp_path):
    two, three = str(tmp_path / 'two'), str(tmp_path / 'three')
    run('calculate-relaxations-from-Ct.py', *CFG1, '-o', two, '-D', '%g %g' % (synth.DISO, synth.DANI))
    txt = run('calculate-relaxations-from-Ct.py', *CFG1, '-o', three, '-D', '%g,%g,0' % (synth.DISO, synth.DANI))
    assert 'fully anisotropic' in txt
    for nm in ('R1', 'R2', 'NOE', 'rho'):
        ok, why = files_equal_numeric(three + '_%s.dat' % nm, two + '_%s.dat' % nm, rtol=1e-6)
        assert ok, (nm, why)


def test_script_rhombic_table_vs_oracle(tmp_path):
    """rhomb = 0.4: the files against the oracle's table written by the project's own writer"""
    out, ref = str(tmp_path / 'rh'), str(tmp_path / 'ref')
    run('calculate-relaxations-from-Ct.py', *CFG1, '-o', out, '-D', '%g %g 0.4' % (synth.DISO, synth.DANI))
    zeta = 0.890023
    R = sd.relaxationModel('NH', 2.0 * np.pi * 600.133e6 / 267.513e6)
    R.set_time_unit('ps')
    ac = fitCt.read_fittedCt_parameters(os.path.join(GOLD, 'cfg1_fittedCt.dat'))
    S2, C, tau, K = ac.get_params_as_arrays()
    h = np.load(os.path.join(GOLD, 'cfg1_vecHistogram.npz'), allow_pickle=True)
    bv, w = sd.convert_LambertCylindricalHist_to_vecs(h['data'], h['edges'])
    n = ac.nModels
    D = hm.ellipsoid_from_iso(synth.DISO, synth.DANI, 0.4)
    tab, _, _ = eo.relax_table(D, R.omega, R.get_f_DD(), R.get_f_CSA(np.repeat(R.gX.csa, n))[None, :], R.time_fact,
                               R.gH.gamma / R.gX.gamma, zeta * S2, zeta * C, tau, K, bv, w, noe_mode=0)
    block = np.transpose(tab[0], (1, 0, 2)).astype(np.float32)            # the float32 datablock the script writes
    spec = importlib.util.spec_from_file_location('relax_from_ct', os.path.join(SCR, 'calculate-relaxations-from-Ct.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    header = mod.print_fitting_params_headers(("Diso", "zeta", "CSA", "chi"), np.multiply((1.0, zeta, 1.0e6, 1.0),
                                              (synth.DISO, 1.0, R.gX.csa, 0.0)), ("ps^-1", "a.u.", "ppm", "a.u."), (False,) * 4)
    resid = [int(k) for k in ac.model.keys()]
    for k, nm in enumerate(('R1', 'R2', 'NOE', 'rho')):
        gs.print_xydy(ref + '_%s.dat' % nm, resid, block[k, :, 0], block[k, :, 1], header=header if k < 3 else "")
        ok, why = files_equal_numeric(out + '_%s.dat' % nm, ref + '_%s.dat' % nm, rtol=1e-6)
        assert ok, (nm, why)
    # and the rhombicity is really in there: the table differs from the symmetric top's
    sym = str(tmp_path / 'sym')
    run('calculate-relaxations-from-Ct.py', *CFG1, '-o', sym, '-D', '%g %g' % (synth.DISO, synth.DANI))
    assert not files_equal_numeric(out + '_R1.dat', sym + '_R1.dat', rtol=1e-6)[0]


def test_script_jomega_rigid_and_refusals(tmp_path):
    out = str(tmp_path / 'jw')
    run('calculate-relaxations-from-Ct.py', *CFG1, '-o', out, '--Jomega', '-D', '%g %g 0.4' % (synth.DISO, synth.DANI))
    assert open(out + '_Jw.dat').read().count('&') == 32
    txt = run('calculate-relaxations-from-Ct.py', '-F', '600.133e6', '-D', '%g 1.26 0.4' % synth.DISO, '--theoretical')
    assert '(x/y/z)' in txt
    r1 = [float(x) for x in txt.split('R1:')[1].split('\n')[0].split()]
    assert len(r1) == 3 and len(set(r1)) == 3          # three distinct axes, three distinct baselines
    txt = run('calculate-relaxations-from-Ct.py', *CFG1, '-o', out, '-D', '%g 1.26 0.4' % synth.DISO, '--opt', 'new', '-e',
              os.path.join(GOLD, 'cfg1_legacy_exp.dat'), expect=1)
    assert 'symmetric top only' in txt


# ---- class API: rsCSA on model-3 statistics, global Drhomb optimisation ----------------------------------------------------
def write_experiments(tmpdir, names, kinds, MHz, vals, errs=None):
    files = []
    for k, (kind, f) in enumerate(zip(kinds, MHz)):
        fn = os.path.join(tmpdir, 'expt_%s_%d.dat' % (kind, round(f)))
        with open(fn, 'w') as fp:
            fp.write('# Type %s\n# NucleiA 15N\n# NucleiB 1H\n# Frequency %.3f\n' % (kind, f))
            for i, nm in enumerate(names):
                fp.write(('%s %.14g\n' % (nm, vals[k][i])) if errs is None else ('%s %.12g %.12g\n' % (nm, vals[k][i], errs[k][i])))
        files.append(fn)
    return files


def test_rscsa_device_search_on_rhombic_statistics(tmp_path):
    """The existing multi-field fixture (tests/golden/cfg1_rscsa.npz) with a rhombic tensor: the one-launch device search
    against scipy's fmin_powell per residue on the host, both on the closed forms of model-3 statistics, held to what
    test_gpu_multifield.py::test_rscsa_device_search_walks_scipy_powell_path demands of the symmetric top -- the fitted CSA to
    2e-3, an uncovered residue untouched, and wherever the two walked the identical path the same call count and the values /
    errors to 1e-14 / 1e-12.  (Its committed count of identical paths is a measured tally of the symmetric-top fixture; no
    such figure is taken from the code under test here.)"""
    import copy
    g = golden('cfg1_rscsa.npz')
    localCt = fitCt.read_fittedCt_parameters(os.path.join(GOLD, 'cfg1_fittedCt.dat'))
    grd = sd.globalRotationalDiffusion_Ellipsoid(D=[synth.DISO, synth.DANI, 0.4])
    grd.import_frame_vectors_npz(os.path.join(GOLD, 'cfg1_vecHistogram.npz'))
    ex = sd.spinRelaxationExperiments(grd, localCt)
    for f in write_experiments(str(tmp_path), localCt.get_names(), [str(k) for k in g['expt_kind']],
                               [float(f) for f in g['expt_MHz']], g['expt_vals'], g['expt_errs']):
        ex.add_experiment(f)
    ex.set_global_zeta(synth.ZETA)
    ex.map_experiment_peaknames_to_models()
    ex.parse_optimisation_params(['rsCSA'])
    ex.eval_all()
    assert grd.kernel_model()[0] == 3
    n = ex.localCtModels.nModels
    start = np.array(ex.get_first_csa(), dtype=float)
    ex.mapExptCoverage[3] = []
    for scale in (1.0, 1.45):
        host, dev = copy.deepcopy(ex), copy.deepcopy(ex)
        host.ctx = dev.ctx = ex.ctx
        for o in (host, dev):
            o.set_all_csa(start * scale)
            o.eval_all()
            o.nObjectiveCalls = 0
        stats = host.rscsa_statistics()
        host.optimisation_loop_do_local_step_host(stats, 0, n)
        dev.optimisation_loop_do_local_step()
        ch, cd = np.array(host.get_first_csa()), np.array(dev.get_first_csa())
        print('scale %g: %d of %d residues on the identical path' % (scale, int((ch == cd).sum()), n))
        np.testing.assert_allclose(cd, ch, rtol=2e-3)
        assert cd[3] == start[3] * scale
        assert not np.allclose(cd[:3], start[:3] * scale, rtol=1e-3)          # the search moved the covered ones
        if (ch == cd).all():
            assert dev.nObjectiveCalls == host.nObjectiveCalls
            for a, b in zip(host.spinrelax, dev.spinrelax):
                np.testing.assert_allclose(b.values, a.values, rtol=1e-14)
                np.testing.assert_allclose(b.errors, a.errors, rtol=1e-12)


def test_global_Drhomb_optimisation_recovers_truth(tmp_path):
    """Noise-free R1 / R2 / NOE targets at two fields for 10 residues from the numpy oracle at (Diso, 1.26, 0.4); the search
    over Diso,Daniso,Drhomb starts at (1.03 Diso, 1.2, 0.2).  Required: chi^2 ends at <= 1e-3 of its start and
    |rhomb - 0.4| <= 0.01.  scipy's Powell with the reference's settings (fmin_powell defaults, direc = diag of the step
    sizes) on the numpy oracle as objective meets both from this start on the CPU (chi^2 12.8 -> 3e-27 in 312 calls, rhomb
    0.4000), so the start asked for, rhomb 0.2, is kept; the GPU-driven run is held to the same two conditions."""
    nsel = 10
    localCt = fitCt.read_fittedCt_parameters(os.path.join(GOLD, 'cfg1_fittedCt.dat'))
    names = localCt.get_names()[:nsel]
    S2, C, tau, K = localCt.get_params_as_arrays()
    h = np.load(os.path.join(GOLD, 'cfg1_vecHistogram.npz'), allow_pickle=True)
    bv, w = sd.convert_LambertCylindricalHist_to_vecs(h['data'], h['edges'])
    kinds, MHz = ['R1', 'R2', 'NOE'] * 2, [600.133] * 3 + [800.0] * 3
    af = [sd.angularFrequencies(fieldStrength=f) for f in (600.133, 800.0)]
    truth, _, _ = eo.relax_table(hm.ellipsoid_from_iso(synth.DISO, 1.26, 0.4), np.array([a.omega for a in af]),
                                 np.array([a.get_factor_DD() for a in af]),
                                 np.array([np.repeat(a.get_factor_CSA(), nsel) for a in af]), 1e-12,
                                 af[0].gB.gamma / af[0].gA.gamma, synth.ZETA * S2[:nsel], synth.ZETA * C[:nsel], tau[:nsel], K[:nsel],
                                 bv, w[:nsel], noe_mode=1)
    vals = [truth[e, :, col, 0] for e in range(2) for col in range(3)]
    grd = sd.globalRotationalDiffusion_Ellipsoid(D=[synth.DISO * 1.03, 1.2, 0.2])
    grd.import_frame_vectors_npz(os.path.join(GOLD, 'cfg1_vecHistogram.npz'))
    ex = sd.spinRelaxationExperiments(grd, localCt)
    for f in write_experiments(str(tmp_path), names, kinds, MHz, vals):
        ex.add_experiment(f)
    ex.set_global_zeta(synth.ZETA)
    ex.map_experiment_peaknames_to_models()
    ex.eval_all()
    chi0 = ex.calc_chisq()
    ex.parse_optimisation_params(['Diso', 'Daniso', 'Drhomb'])
    chisq = ex.perform_optimisation()
    print('chi^2 %g -> %g in %d calls; Diso %g Daniso %g Drhomb %g' % (chi0, chisq, ex.nObjectiveCalls, ex.get_global_Diso(),
                                                                      ex.get_global_Daniso(), ex.get_global_Drhomb()))
    assert chisq <= 1e-3 * chi0
    assert abs(ex.get_global_Drhomb() - 0.4) <= 0.01
    # written with the other globals
    ex.export_xvg(str(tmp_path / 'opt'))
    txt = open(str(tmp_path / 'opt_15N1H_600MHz_R1.xvg')).read()
    assert '# Optimised Drhomb: 0.4' in txt and '# Optimised Daniso: 1.26' in txt


def test_multi_field_script_three_values(tmp_path):
    localCt = fitCt.read_fittedCt_parameters(os.path.join(GOLD, 'cfg1_fittedCt.dat'))
    names = localCt.get_names()
    files = write_experiments(str(tmp_path), names, ['R1', 'NOE'], [600.133, 600.133], np.ones((2, len(names))))
    common = ['-f', os.path.join(GOLD, 'cfg1_fittedCt.dat'), '--distfn', os.path.join(GOLD, 'cfg1_vecHistogram.npz')]
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    D = hm.ellipsoid_from_iso(synth.DISO, 1.26, 0.4)
    run('calculate-relaxations-multi-field.py', *common, '-o', a, '-D', '%.12g %.12g %.12g' % D, *files)
    run('calculate-relaxations-multi-field.py', *common, '-o', b, '-D', '%g' % synth.DISO, '--aniso', '1.26', '--rhomb', '0.4', *files)
    for nm in ('R1', 'NOE'):
        fa, fb = (p + '_15N1H_600MHz_%s.xvg' % nm for p in (a, b))
        assert '# Fixed Drhomb: 0.4 a.u.' in open(fb).read()
        ok, why = files_equal_numeric(fa, fb, rtol=1e-5)
        assert ok, why
